"""Deviation of every read's alignment from its guide on the GPU (sa_guide_deviation_records, sa_batch_guide_deviation): every
field must equal the restatement in deviation_ref.py, with the LDS window (SA_DEV_WINDOW) and without it (SA_DEV_DIRECT, the default) alike, over the smallest shapes at
which the kernels can go wrong, all of them separate jobs of one call; and chained onto a finished batch the call equals
guide_deviation_records fed from the same batch's pairs."""
import numpy as np
import pytest

import signalalign_amd as sa

import sa_cases as cases
import deviation_ref as ref

pytestmark = pytest.mark.gpu

READ_FIELDS = ("status", "n_sets", "set_first", "n_aligned", "n_flagged", "n_on_mea", "sum_abs", "max_abs", "max_abs_mea", "max_event")
SET_FIELDS = ("first_event", "last_event", "count", "peak", "mea_peak", "center_event", "open_end")


def _job(ax, ay, n_events, x, y, prob_e7=None, mea=(), rng=None):
    x, y = np.asarray(x, dtype=np.int32), np.asarray(y, dtype=np.int32)
    if prob_e7 is None:
        prob_e7 = rng.integers(0, 4, size=len(x)) * 2500000 + rng.integers(0, 2, size=len(x))   # few values: many ties
    return dict(ax=np.asarray(ax, dtype=np.int64), ay=np.asarray(ay, dtype=np.int64), n_events=int(n_events), x=x, y=y,
                prob_e7=np.asarray(prob_e7, dtype=np.int64), mea=sorted(int(e) for e in mea))


AX, AY = [1000, 1040, 1100, 1300], [3, 40, 100, 300]      # the guide of the jobs made from a list of differences


def _from_diffs(diffs, rng, mea=(), ax=AX, ay=AY):
    """one record per event whose entry in diffs is not None, at guide + the entry"""
    ys = [y for y, d in enumerate(diffs) if d is not None]
    xs = [ref.guide_position(ax, ay, y) + diffs[y] for y in ys]
    return _job(ax, ay, len(diffs), xs, ys, rng=rng, mea=mea)


def _random_job(rng, n_events, n_records, n_anchors, spread=30):
    ay = np.sort(rng.choice(n_events, size=n_anchors, replace=False)) if n_anchors else np.zeros(0, dtype=np.int64)
    ax = 500 + 2 * ay + rng.integers(0, 2, size=n_anchors)
    y = np.sort(rng.integers(0, n_events, size=n_records))
    g = np.array([ref.guide_position(ax, ay, int(v)) if n_anchors else 500 for v in y], dtype=np.int64)
    x = np.maximum(g + rng.integers(-spread, spread + 1, size=n_records), 0)
    return _job(ax, ay, n_events, x, y, rng=rng, mea=rng.choice(n_events, size=n_events // 3, replace=False))


def _diagonal_job(rng, n_records):
    """records ordered by x + y as a batch leaves them, two per event, drifting away from the guide and back"""
    y = np.arange(n_records) // 2
    n_events = int(y[-1]) + 1
    ax, ay = [200, 200 + n_events], [0, n_events]        # (the last anchor lies behind the last event)
    drift = (40 * np.sin(np.arange(n_records) / 150.0)).astype(np.int64)
    x = 200 + y // 2 + drift + (np.arange(n_records) & 1)
    return _job(ax, ay, n_events, x, y, rng=rng, mea=range(0, n_events, 3))


def _shape_jobs():
    rng = np.random.default_rng(11)
    D = lambda diffs, **kw: _from_diffs(diffs, rng, **kw)
    wave = lambda n: [int(v) for v in rng.integers(-25, 26, size=n)]
    jobs = [
        _random_job(rng, 50, 30, 4),
        _job(AX, AY, 50, [], [], []),                                        # no record, among others
        _random_job(rng, 50, 30, 0),                                         # no anchors: no guide
        _random_job(rng, 50, 30, 1),                                         # a single anchor
        _job(AX, AY, 50, [1234], [17], [5]),                                 # a single record
        _diagonal_job(rng, 4095), _diagonal_job(rng, 4096), _diagonal_job(rng, 4097),   # the chunk boundary
        D(wave(63)), D(wave(64)), D(wave(65)), D(wave(129)),                 # the wave step
        D([0] * 60 + [20] * 10 + [0] * 130),                                 # a run that crosses a step boundary
        D([0] * 60 + [-20] * 140 + [0] * 10, mea=[70, 199]),                 # ... and two of them
        D([0] * 63 + [20] + [0] * 10), D([0] * 64 + [20] + [0] * 10),        # runs of length 1 at a step's two ends
        D([0, 0, 11, 0, 0, 10, 0]),                                          # a run of length 1; 10 is not above the threshold
        D([15] * 130, mea=[129]),                                            # every event flagged: one open set
        D([0] * 9 + [30]), D([0] * 8 + [30, 0]),                             # a run ending on the last event, and one before it
        D([0] * 63 + [30]), D([0] * 127 + [30] * 2), D([0] * 62 + [30, 0]),
        D([0, 20, None, 20, 20, None, None, 0, 20, None], mea=[2, 3, 9]),    # unaligned events inside a run, and on the path
        D([None] * 70 + [20] + [None] * 70 + [20, 0]),                       # ... a whole step of them
        _job(AX, AY, 20, [1000, 1030, 1020], [5, 5, 5], [777, 777, 776]),    # equal prob_e7, different x: the largest x
        _job(AX, AY, 20, [1050, 1001, 1002, 1060], [5, 5, 6, 6], [0, 0, 10 ** 7, 0]),   # prob_e7 of 0 and of 1e7
        _job(AX, AY, 20, [1000] * 5 + [1030] * 5, [7] * 10, [5] * 10),       # several records with the same (x, y)
        _job([100, 30000], [0, 20000], 20001, np.tile([100, 20000], 100), np.tile([0, 20000], 100), rng=rng),   # y jumps past any window
        D([0, 319, 320, 5000, 0], ax=[200000], ay=[2]),               # abs beyond the last bucket
        D([0, -150000, 0], ax=[200000], ay=[1]),
    ]
    for _ in range(40):
        jobs.append(_random_job(rng, 30, 25, int(rng.integers(1, 6))))
    return jobs


_SHARED = {}


def _shapes():
    """the shape jobs as the arrays of one call, computed once"""
    if not _SHARED:
        jobs = _shape_jobs()
        first = np.concatenate([[0], np.cumsum([len(j["x"]) for j in jobs])]).astype(np.int64)
        cat = lambda f, dt: np.concatenate([j[f] for j in jobs]).astype(dt)
        _SHARED["call"] = (jobs, first, cat("x", np.int32), cat("y", np.int32), cat("prob_e7", np.int64))
        _SHARED["exp"] = {}
    return _SHARED["call"]


def _expected(params, with_mea=True):
    jobs, first, x, y, p = _shapes()
    key = (params, with_mea)
    if key not in _SHARED["exp"]:
        mea = [j["mea"] for j in jobs] if with_mea else None
        _SHARED["exp"][key] = ref.deviation(jobs, first, x.tolist(), y.tolist(), p.tolist(), mea=mea, threshold=params[0],
                                            bucket_size=params[1], n_buckets=params[2])
    return _SHARED["exp"][key]


def _mea_arg(jobs):
    return [np.array([(0, e) for e in j["mea"]], dtype=np.int32).reshape(-1, 2) for j in jobs]


def _check(got, exp, jobs, threshold):
    for f in READ_FIELDS:
        assert got["reads"][f].tolist() == [r[f] for r in exp["reads"]], f
    assert (got["reads"]["pad"] == 0).all() and (got["sets"]["pad"] == 0).all()
    assert len(got["sets"]) == len(exp["sets"])
    for f in SET_FIELDS:
        assert got["sets"][f].tolist() == [s[f] for s in exp["sets"]], f
    assert got["hist"].tolist() == exp["hist"]
    assert got["total_hist"].tolist() == exp["total_hist"]
    # the two properties: every row sums to n_aligned, and the summed histogram is the sum of the rows
    assert got["hist"].sum(axis=1).tolist() == got["reads"]["n_aligned"].tolist()
    assert got["total_hist"].tolist() == got["hist"].astype(np.int64).sum(axis=0).tolist()
    if "events" in got:
        want = np.zeros(sum(j["n_events"] for j in jobs), dtype=sa.DEVIATION_EVENT_DTYPE)
        at = 0
        for j, rows in zip(jobs, exp["rows"]):
            for r in rows:
                want[at + r["y"]] = (r["best_x"], r["guide"], r["diff"], 1 | (2 if r["on_mea"] else 0) | (4 if r["flagged"] else 0))
            at += j["n_events"]
        assert got["events"].tobytes() == want.tobytes()


PARAMS = [(10, 5, 64), (10, 5, 1), (10, 1, 1024), (0, 5, 64)]


@pytest.mark.parametrize("params", PARAMS)
def test_shapes_with_and_without_the_window(params):
    jobs, first, x, y, p = _shapes()
    exp = _expected(params)
    # what the shapes are there for is there
    if params == PARAMS[0]:
        st = [r["status"] for r in exp["reads"]]
        assert st[1] == ref.NO_RECORDS and st[2] == ref.NO_GUIDE and st.count(0) == len(st) - 2
        assert [len(j["x"]) for j in jobs[5:8]] == [4095, 4096, 4097] and [j["n_events"] for j in jobs[8:12]] == [63, 64, 65, 129]
        assert any(s["first_event"] < 64 <= s["last_event"] for s in exp["sets"]) and any(s["count"] == 1 for s in exp["sets"])
        assert any(s["open_end"] and s["count"] == 130 for s in exp["sets"]) and max(r["max_abs"] for r in exp["reads"]) >= 150000
        assert exp["total_hist"][63] >= 4 and sum(r["n_sets"] for r in exp["reads"]) > 60
    results = []
    for flags in (sa.DEV_EVENTS | sa.DEV_WINDOW, sa.DEV_EVENTS | sa.DEV_DIRECT, sa.DEV_EVENTS):
        got = sa.guide_deviation_records(jobs, first, x, y, p, mea=_mea_arg(jobs), params=params, flags=flags)
        _check(got, exp, jobs, params[0])
        assert got["kernel_ms"] > 0
        results.append(got)
    for f in ("reads", "sets", "hist", "total_hist", "events"):
        assert results[0][f].tobytes() == results[1][f].tobytes() == results[2][f].tobytes(), f


def test_without_a_path_and_without_the_events():
    jobs, first, x, y, p = _shapes()
    got = sa.guide_deviation_records(jobs, first, x, y, p)
    assert "events" not in got
    _check(got, _expected(PARAMS[0], with_mea=False), jobs, 10)
    assert (got["reads"]["n_on_mea"] == 0).all() and (got["sets"]["mea_peak"] == 0).all()
    # dropping the sets that are open at the end gives the reference's list
    exp = _expected(PARAMS[0], with_mea=False)
    like_ref = ref.deviation(jobs, first, x.tolist(), y.tolist(), p.tolist(), drop_open_sets=True)
    kept = got["sets"][got["sets"]["open_end"] == 0]
    assert len(kept) == len(like_ref["sets"]) < len(exp["sets"])
    for f in SET_FIELDS:
        assert kept[f].tolist() == [s[f] for s in like_ref["sets"]], f
    # no job at all
    none = sa.guide_deviation_records([], [0], [], [], [], flags=sa.DEV_EVENTS)
    assert len(none["reads"]) == 0 and len(none["sets"]) == 0 and len(none["events"]) == 0 and not none["total_hist"].any()
    sa.guide_deviation_release()


# ---- chained onto a real batch ------------------------------------------------------------------------------------------------
def _batch(jobs, flags=0, run=True):
    pm = sa.Model.load(cases.MODEL_6MER)
    b = sa.Batch(pm, sa.default_params(), jobs, flags=flags)
    if run:
        b.run()
    return b


def test_chained_onto_a_batch_equals_the_records_of_its_pairs():
    jobs = cases.realistic_anchor_jobs(cases.MODEL_6MER, 3, 600, 700)
    assert all(len(j["ax"]) < 300 for j in jobs)                              # sparse anchors: the guide is interpolated
    djobs = [dict(ax=j["ax"], ay=j["ay"], n_events=len(j["events"])) for j in jobs]
    b16 = _batch(jobs)
    paths = [m[0] for m in b16.mea()]
    assert all(len(m) > 300 for m in paths)
    rows, first = b16.pairs_all()
    assert first[-1] > 1500
    b8 = _batch(jobs, sa.FLAG_PAIRS8)
    for mea in (paths, None):
        events = None if mea is None else [m[:, 1].tolist() for m in mea]
        exp = ref.deviation(djobs, first, rows["x"].tolist(), rows["y"].tolist(), rows["prob_e7"].tolist(), mea=events)
        assert sum(r["n_aligned"] for r in exp["reads"]) > 1500
        from_records = sa.guide_deviation_records(djobs, first, rows["x"], rows["y"], rows["prob_e7"], mea=mea, flags=sa.DEV_EVENTS)
        _check(from_records, exp, djobs, 10)
        for b in (b16, b8):
            for flags in (sa.DEV_EVENTS | sa.DEV_WINDOW, sa.DEV_EVENTS | sa.DEV_DIRECT):
                got = sa.batch_guide_deviation(b, jobs, mea=mea, flags=flags)
                for f in ("reads", "sets", "hist", "total_hist", "events"):
                    assert got[f].tobytes() == from_records[f].tobytes(), f
    # the 8-byte batch holds the same (x, y, prob_e7) as the 16-byte one, so one expectation serves both
    r8 = b8.pairs8(1)
    assert np.array_equal(r8["x"], rows["x"][first[1]:first[2]]) and np.array_equal(r8["prob_e7"], rows["prob_e7"][first[1]:first[2]])
    want = sa.batch_guide_deviation(b16, jobs, mea=paths)
    b16.release_device()                                                      # the records go up again
    again = sa.batch_guide_deviation(b16, jobs, mea=paths)
    for f in ("reads", "sets", "hist", "total_hist"):
        assert again[f].tobytes() == want[f].tobytes(), f
    b16.close()
    b8.close()


def test_batch_refusals():
    jobs = cases.realistic_anchor_jobs(cases.MODEL_6MER, 2, 200, 710)

    def refused(b, code, the_jobs=jobs):
        with pytest.raises(sa.SaError) as e:
            sa.batch_guide_deviation(b, the_jobs)
        assert e.value.code == code

    b = _batch(jobs, run=False)
    refused(b, -7)                                                            # SA_ESTATE: not run
    b.run()
    refused(b, -1, jobs[:1])                                                  # not the batch's number of jobs
    refused(b, -1, [jobs[0], dict(ax=jobs[1]["ax"], ay=jobs[1]["ay"], n_events=199)])   # not the batch's n_events
    assert sa.batch_guide_deviation(b, jobs)["reads"]["n_aligned"].min() > 100
    b.close()
    with_x = [dict(j, ref=j["ref"][:60] + "X" + j["ref"][61:]) for j in jobs]
    b = sa.Batch(sa.Model.load(cases.MODEL_6MER), sa.default_params(), with_x, ambig=sa.default_ambig({"X": "ACGT"}), flags=sa.FLAG_VC_ROWS)
    b.run()
    refused(b, -1)                                                            # SA_EINVAL: rows dropped
    b.close()
