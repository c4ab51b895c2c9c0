"""Call quality on the GPU (sa_call_quality_records, sa_batch_call_quality) against the restatement in Python integers
(call_quality_ref.py), exactly: the hand-worked table; the sizes at which a wave, a tile of sites, a chunk of records or the scan
takes another path; calls outside the guide on either side and strand; the histogram's edges; the gaps' edges; labels from the read
and from the positions table; the same bytes twice, with the jobs permuted and without the LDS window; the argument checks; then
the call chained onto a small SA_FLAG_SITE_CALLS batch against the records call fed with the batch's own pairs, site calls and
anchors."""
import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import call_quality_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

SA_EINVAL, SA_ESTATE = -1, -7
THRESHOLD = 0.5
READ_FIELDS = [n for n in sa.CALLQ_READ_DTYPE.names]
CALL_FIELDS = [n for n in sa.CALLQ_CALL_DTYPE.names if n != "pad"]


@pytest.fixture(scope="module")
def acc():
    """letters "CE", threshold 0.5, and a positions table: on contig 0 every position that is no multiple of 3, strand by parity
    of the position's tens, the letter by parity of the position"""
    truth = [(0, r, (r // 10) % 2, "CE"[r % 2]) for r in range(0, 20000) if r % 3]
    a = sa.CallScores("CE", truth=truth, n_bins=10, threshold=THRESHOLD)
    a.table = {(c, r, s): "CE".index(l) for c, r, s, l in truth}
    yield a
    a.close()


def make_job(rng, n_events=40, n_anchors=5, n_sites=6, n_path=20, x_sign=1, true_letter=-1, recs_per_site=3, other=0.0, mapped=0):
    lengths = rng.integers(1, 10, size=n_events)
    holes = np.where(rng.random(n_events) < 0.2, rng.integers(1, 60, size=n_events), 0)
    raw_start = np.cumsum(np.concatenate([[int(rng.integers(0, 50))], (lengths + holes)[:-1]])) if n_events else np.zeros(0, dtype=np.int64)
    ay = np.sort(rng.choice(n_events, size=n_anchors, replace=False)) if n_anchors else np.zeros(0, dtype=np.int64)
    ax = np.cumsum(rng.integers(0, 4, size=n_anchors)) + 3 if n_anchors else np.zeros(0, dtype=np.int64)
    span = max(int(ax[-1]) + 4 if n_anchors else 8, 2 * n_sites)          # sites before the first and after the last guide row
    site_x = np.sort(rng.choice(span, size=n_sites, replace=False))
    rec_x, rec_y = [], []
    for x in site_x:
        n = recs_per_site if isinstance(recs_per_site, int) else int(rng.integers(*recs_per_site))
        rec_x += [int(x)] * n
        rec_y += [int(y) for y in rng.integers(0, n_events, size=n)]
    stray = [int(x) for x in rng.choice(span + 5, size=min(8, span)) if x not in set(site_x.tolist())]
    rec_x += stray
    rec_y += [int(y) for y in rng.integers(0, max(n_events, 1), size=len(stray))] if n_events else []
    order = rng.permutation(len(rec_x))
    p = rng.choice([0.0, 0.25, 0.5, np.nextafter(0.5, 1.0), 0.75, 1.0], size=n_sites)
    x0 = int(rng.integers(5000, 9000))
    return dict(job_map=dict(contig=0, x_sign=x_sign, x0=x0, strand=int(rng.integers(0, 2)), mapped_strand=mapped, true_letter=true_letter),
                job=dict(ax=ax, ay=ay, raw_start=raw_start, raw_length=lengths),
                site_x=site_x, site_prob=np.stack([p, 1.0 - p], axis=1) if n_sites else np.zeros((0, 2)),
                site_other=(rng.random(n_sites) < other).astype(np.uint8),
                rec_x=np.array(rec_x, dtype=np.int32)[order], rec_y=np.array(rec_y, dtype=np.int32)[order],
                path=np.sort(rng.choice(n_events, size=n_path, replace=False)) if n_path else None)


def flat(jobs):
    first = lambda key: np.concatenate([[0], np.cumsum([len(j[key]) for j in jobs])]).astype(np.int64)
    cat = lambda key, dt, w=1: np.concatenate([np.asarray(j[key], dtype=dt).reshape(-1, w) for j in jobs] + [np.zeros((0, w), dtype=dt)])
    return dict(site_first=first("site_x"), site_x=cat("site_x", np.int32).ravel(), site_prob=cat("site_prob", np.float64, 2),
                site_other=cat("site_other", np.uint8).ravel(), rec_first=first("rec_x"), rec_x=cat("rec_x", np.int32).ravel(),
                rec_y=cat("rec_y", np.int32).ravel())


def run(acc, jobs, params=None, flags=sa.CQ_CALLS, with_paths=True):
    f = flat(jobs)
    mea = None
    if with_paths:
        mea = [None if j["path"] is None else np.stack([np.zeros(len(j["path"]), dtype=np.int32), j["path"]], axis=1) for j in jobs]
    return sa.call_quality_records(acc, [j["job_map"] for j in jobs], [j["job"] for j in jobs], f["site_first"], f["site_x"],
                                   f["site_prob"], f["rec_first"], f["rec_x"], f["rec_y"], site_other=f["site_other"], mea=mea,
                                   params=params, flags=flags)


def expect(acc, jobs, params=None):
    f = flat(jobs)
    return ref.call_quality_jobs([j["job_map"] for j in jobs], [j["job"] for j in jobs], f["site_first"], f["site_x"], f["site_prob"],
                                 f["rec_first"], f["rec_x"], f["rec_y"], [j["path"] for j in jobs], THRESHOLD, acc.table,
                                 site_other=f["site_other"], params=params or ref.DEFAULT_PARAMS)


def check(acc, jobs, params=None, flags=sa.CQ_CALLS):
    """the call against the restatement, field by field; returns both"""
    got = run(acc, jobs, params, flags)
    reads, calls, gaps, hists, total = expect(acc, jobs, params)
    assert len(got["reads"]) == len(reads)
    for j, (g, e) in enumerate(zip(got["reads"], reads)):
        assert {n: int(g[n]) for n in READ_FIELDS} == e, j
    assert len(got["calls"]) == len(calls)
    for g, e in zip(got["calls"], calls):
        assert {n: (float(g[n]) if n == "prob_true" else int(g[n])) for n in CALL_FIELDS} == e
    assert [(int(g["y_before"]), int(g["y_after"]), int(g["gap"])) for g in got["gaps"]] == gaps
    assert (got["total_hist"] == total).all()
    for j, h in enumerate(hists):
        assert (got["hist"][j] == h).all(), j
    assert got["total_hist"].sum() == sum(r["n_calls"] - r["n_outside"] for r in reads)
    return got, reads


def hand_job():
    h = ref.HAND
    return dict(job_map=h["job_map"], job=h["job"], site_x=h["site_x"], site_prob=np.array(h["site_prob"]), site_other=np.zeros(4, dtype=np.uint8),
                rec_x=h["rec_x"], rec_y=h["rec_y"], path=np.array(h["path_y"]))


def test_hand_worked_table(acc):
    got, reads = check(acc, [hand_job()])
    r = got["reads"][0]
    assert (int(r["n_calls"]), int(r["n_correct"]), int(r["n_outside"]), int(r["max_abs_delta2"]), int(r["max_x"])) == (4, 2, 2, 96, 7)
    assert [int(d) for d in got["calls"]["delta2"]] == [0, 1, 96, 0] and [int(c) for c in got["calls"]["correct"]] == [1, 0, 1, 0]
    assert got["kernel_ms"] > 0 and sum(sa.call_quality_last_kernel_ms().values()) > 0
    # without SA_CQ_CALLS: the same reads but for call_first, no calls
    bare = run(acc, [hand_job()], flags=0)
    assert "calls" not in bare and bare["reads"].tobytes() == got["reads"].tobytes()


def test_sites_per_job_at_the_edges_of_a_wave_and_of_a_tile(acc):
    rng = np.random.default_rng(1)
    jobs = [make_job(rng, n_sites=n, x_sign=s, recs_per_site=1) for n, s in ((0, 1), (1, -1), (63, 1), (64, -1), (65, 1), (1023, 1),
                                                                              (1024, -1), (1025, 1), (4097, -1))]
    got, reads = check(acc, jobs)
    assert reads[0]["status"] & ref.NO_SITES and [r["n_calls"] + r["n_unlabelled"] for r in reads] == [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
    assert sum(r["n_unlabelled"] for r in reads) > 1000 and sum(r["n_outside"] for r in reads) > 1000


def test_records_per_job_at_the_edges_of_a_chunk_all_on_one_site(acc):
    rng = np.random.default_rng(2)
    jobs = [make_job(rng, n_events=300, n_sites=1, recs_per_site=n, true_letter=0) for n in (4095, 4096, 4097, 8200)]
    for flags in (sa.CQ_CALLS, sa.CQ_CALLS | sa.CQ_BAND_DIRECT):
        got, reads = check(acc, jobs, flags=flags)
        assert [r["n_calls"] for r in reads] == [1, 1, 1, 1]
        assert all(int(c["raw_length"]) > 500 for c in got["calls"])          # (the band spans nearly the whole read)


@pytest.mark.parametrize("x_sign", [1, -1])
def test_guides_of_no_one_and_two_rows_and_calls_outside_them(acc, x_sign):
    rng = np.random.default_rng(3 + x_sign)
    jobs = [make_job(rng, n_anchors=n, n_sites=12, x_sign=x_sign, true_letter=1) for n in (0, 1, 2, 5)]
    # a guide whose rows share an anchor_x, with a call at it, before the first and after the last
    dup = make_job(rng, n_anchors=4, n_sites=0, x_sign=x_sign, true_letter=0)
    dup["job"]["ax"] = np.array([4, 6, 6, 9])
    dup.update(site_x=np.array([2, 4, 5, 6, 7, 9, 11]), site_prob=np.tile([0.6, 0.4], (7, 1)), site_other=np.zeros(7, dtype=np.uint8),
               rec_x=np.array([2, 4, 5, 6, 7, 9, 11], dtype=np.int32), rec_y=np.arange(7, dtype=np.int32))
    got, reads = check(acc, jobs + [dup])
    assert reads[0]["status"] & ref.NO_GUIDE and reads[0]["n_outside"] == reads[0]["n_calls"] == 12 and reads[0]["max_x"] == -1
    c = got["calls"][int(got["reads"]["call_first"][4]):]
    assert [int(v) for v in c["outside"]] == ([1, 0, 0, 0, 0, 0, 1] if x_sign > 0 else [1, 0, 0, 0, 0, 0, 1])
    ay = dup["job"]["ay"]
    assert int(c["guide_event"][3]) == int(ay[1] if x_sign > 0 else ay[2])      # of two rows at x = 6 the one the walk meets first
    assert int(c["guide_event"][2]) == int(ay[0] if x_sign > 0 else ay[1])      # x = 5: the row before it in reference order


def delta_job(d, x_sign=1):
    """one call whose delta2 is exactly d: the guide's event has its middle at sample 1001 (1000..1001, or 999..1002 when the band
    itself starts at 1000), the band is one event"""
    mid2 = 2002 + d
    b_len = 2 if mid2 % 2 == 0 else 1
    b_start = (mid2 - b_len) // 2
    band_first = b_start < 1000
    g_start, g_len = (999, 4) if b_start == 1000 else (1000, 2)
    rs, rl = ([b_start, g_start], [b_len, g_len]) if band_first else ([g_start, b_start], [g_len, b_len])
    return dict(job_map=dict(contig=0, x_sign=x_sign, x0=50, strand=0, mapped_strand=0, true_letter=0),
                job=dict(ax=[5], ay=[1 if band_first else 0], raw_start=rs, raw_length=rl), site_x=[5], site_prob=np.array([[0.9, 0.1]]),
                site_other=np.zeros(1, dtype=np.uint8), rec_x=[5], rec_y=[0 if band_first else 1], path=None)


def test_histogram_edges_and_the_floor_of_negative_deltas(acc):
    ds = [-9, -7, -6, -5, -3, -2, -1, 0, 1, 9, 10, 11, 400]
    jobs = [delta_job(d, 1 if i % 2 else -1) for i, d in enumerate(ds)]
    got, reads = check(acc, jobs, params=(-3, 2, 4, 30))
    assert [int(c["delta2"]) for c in got["calls"]] == ds
    # 2 * bin_lo = -6, bins of 4: underflow below -6, slot 1 from -6, the last inside value 9, overflow from 10
    slots = [int(np.flatnonzero(h.sum(axis=1))[0]) for h in got["hist"]]
    assert slots == [0, 0, 1, 1, 1, 2, 2, 2, 2, 4, 5, 5, 5]
    for params in ((-3, 2, 1, 30), (-10000, 100, 1024, 30), (0, 1, 1024, 30), (-1, 1, 1, 30)):
        check(acc, jobs, params=params)
    got, _ = check(acc, jobs, params=(-1, 1, 1, 30))                 # one bin, [-2, 0)
    assert [int(v) for v in got["total_hist"].sum(axis=1)] == [5, 2, 6]


def test_paths_at_the_edges_of_a_wave_and_gaps_at_the_edges_of_min_gap(acc):
    rng = np.random.default_rng(5)
    n_events = 200
    lengths = np.full(n_events, 5)
    holes = np.zeros(n_events, dtype=np.int64)
    holes[9], holes[19], holes[63], holes[127] = 30, 31, 31, 45          # before events 10, 20, 64 and 128
    raw_start = np.cumsum(np.concatenate([[0], (lengths + holes)[:-1]]))
    jobs = []
    for n_path in (0, 1, 63, 64, 65, 129, 200):
        j = make_job(rng, n_events=n_events, n_path=0, true_letter=0)
        j["job"]["raw_start"], j["job"]["raw_length"] = raw_start, lengths
        j["path"] = np.arange(n_path) if n_path else None
        jobs.append(j)
    sparse = make_job(rng, n_events=n_events, n_path=0, true_letter=0)
    sparse["job"]["raw_start"], sparse["job"]["raw_length"] = raw_start, lengths
    sparse["path"] = np.arange(0, n_events, 7)                           # every pair skips six events: 30 samples, or more over a hole
    jobs.append(sparse)
    got, reads = check(acc, jobs)
    assert [r["n_gaps"] for r in reads[:7]] == [0, 0, 1, 1, 2, 3, 3] and reads[0]["status"] & ref.NO_PATH
    g = got["gaps"][int(got["reads"]["gap_first"][5]):][:3]
    assert [(int(a["y_before"]), int(a["y_after"]), int(a["gap"])) for a in g] == [(19, 20, 31), (63, 64, 31), (127, 128, 45)]
    got0, reads0 = check(acc, jobs, params=(-10000, 100, 200, 0))
    assert [r["n_gaps"] for r in reads0[:7]] == [0, 0, 2, 2, 3, 4, 4]      # (contiguous events: a gap of 0 is none)
    assert reads0[7]["n_gaps"] == reads0[7]["n_path"] - 1 and reads[7]["n_gaps"] == 4


@pytest.mark.parametrize("n_jobs", [1, 255, 257, 1100])
def test_job_counts_with_mixed_labels(acc, n_jobs):
    rng = np.random.default_rng(n_jobs)
    jobs = []
    for j in range(n_jobs):
        jobs.append(make_job(rng, n_events=int(rng.integers(12, 30)), n_anchors=int(rng.integers(0, 6)),
                             n_sites=0 if j % 50 == 7 else int(rng.integers(1, 9)), n_path=0 if j % 50 == 9 else 10,
                             x_sign=int(rng.choice([1, -1])), true_letter=int(rng.choice([-1, -1, 0, 1])), recs_per_site=(1, 5),
                             other=0.2, mapped=int(rng.integers(0, 2))))
    got, reads = check(acc, jobs)
    if n_jobs > 1:
        assert sum(r["n_unlabelled"] for r in reads) > 20 and sum(r["n_other_sites"] for r in reads) > 20
        assert sum(r["n_correct"] for r in reads) > 20 and sum(r["n_outside"] for r in reads) > 20
        assert any(r["status"] & ref.NO_SITES for r in reads) and any(r["status"] & ref.NO_PATH for r in reads)
        # the same call again, without the LDS window, and with the jobs permuted: the same bytes per job
        again = run(acc, jobs)
        direct = run(acc, jobs, flags=sa.CQ_CALLS | sa.CQ_BAND_DIRECT)
        for other in (again, direct):
            assert all(other[k].tobytes() == got[k].tobytes() for k in ("reads", "calls", "gaps", "hist", "total_hist"))
        perm = rng.permutation(n_jobs)
        shuffled = run(acc, [jobs[q] for q in perm])
        assert shuffled["total_hist"].tobytes() == got["total_hist"].tobytes()
        for at, q in enumerate(perm):
            a, b = shuffled["reads"][at], got["reads"][q]
            same = [n for n in READ_FIELDS if n not in ("call_first", "gap_first")]
            assert [int(a[n]) for n in same] == [int(b[n]) for n in same]
            ca = shuffled["calls"][int(a["call_first"]):int(a["call_first"] + a["n_calls"])]
            cb = got["calls"][int(b["call_first"]):int(b["call_first"] + b["n_calls"])]
            ga = shuffled["gaps"][int(a["gap_first"]):int(a["gap_first"] + a["n_gaps"])]
            gb = got["gaps"][int(b["gap_first"]):int(b["gap_first"] + b["n_gaps"])]
            assert ca.tobytes() == cb.tobytes() and ga.tobytes() == gb.tobytes()
            assert shuffled["hist"][at].tobytes() == got["hist"][q].tobytes()


def refused(acc, job, code=SA_EINVAL, **kw):
    with pytest.raises(sa.SaError) as e:
        run(acc, [job], **kw)
    assert e.value.code == code


def test_argument_checks(acc):
    rng = np.random.default_rng(9)
    good = make_job(rng, true_letter=0)
    run(acc, [good])

    def bad(**change):
        j = dict(good)
        j["job"] = dict(good["job"])
        j["job_map"] = dict(good["job_map"])
        for key, value in change.items():
            where = j["job"] if key in j["job"] else j["job_map"] if key in j["job_map"] else j
            where[key] = value
        return j
    rs, rl, ax, ay = (np.array(good["job"][k]) for k in ("raw_start", "raw_length", "ax", "ay"))
    for params in ((0, 0, 10, 30), (0, 1, 0, 30), (0, 1, 1025, 30), (0, 1, 10, -1), (2 ** 41, 1, 10, 30), (0, 2 ** 41, 10, 30)):
        refused(acc, good, params=params)
    refused(acc, good, flags=8)
    neg, same, zero = rs.copy(), rs.copy(), rl.copy()
    neg[0], same[5], zero[3] = -1, rs[4], 0
    for change in (dict(raw_start=neg), dict(raw_start=same), dict(raw_length=zero), dict(ay=ay[::-1].copy()), dict(ax=ax[::-1].copy() + 1),
                   dict(ax=np.where(np.arange(len(ax)) == len(ax) - 1, 2 ** 28, ax)), dict(ay=np.where(np.arange(len(ay)) == len(ay) - 1, len(rs), ay)),
                   dict(path=np.array([3, 3, 4])), dict(path=np.array([5, 4])), dict(path=np.array([0, len(rs)])),
                   dict(x_sign=0), dict(strand=2), dict(mapped_strand=-1), dict(true_letter=2), dict(contig=-1),
                   dict(site_x=good["site_x"][::-1].copy()), dict(site_prob=np.where(np.arange(12).reshape(6, 2) == 3, np.nan, good["site_prob"])),
                   dict(site_prob=good["site_prob"] + 1.0), dict(rec_y=np.full(len(good["rec_y"]), len(rs), dtype=np.int32)),
                   dict(rec_x=np.full(len(good["rec_x"]), int(good["site_x"][0]), dtype=np.int32))):      # (sites with no record of their x)
        refused(acc, bad(**change))
    far = rs.copy()
    far[-1] = 2 ** 31
    refused(acc, bad(raw_start=far), code=-8)
    run(acc, [good])                                                    # (a refused call leaves nothing behind)


def chained_inputs():
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 3, 600, 40, cpg_ambiguous=True)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 2, 600, 50, cpg_ambiguous=True, cpg_every=3)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 1, 500, 60)                                       # no site
    jobs += cases.thin_anchors_like_a_guide_alignment(cases.synthetic_jobs(cases.MODEL_CPG, 1, 900, 70, cpg_ambiguous=True, cpg_every=3))
    out = []
    for q, j in enumerate(jobs):
        n = len(j["events"])
        lengths = 3 + (np.arange(n) * 7 + q) % 6
        holes = np.where(np.arange(n) % 53 == 52, 40, 0)
        out.append(dict(ax=j["ax"], ay=j["ay"], raw_length=lengths, raw_start=np.cumsum(np.concatenate([[q], (lengths + holes)[:-1]]))))
    return jobs, out


def test_chained_onto_a_batch_equals_the_records_call_fed_from_the_batch(acc):
    jobs, cq_jobs = chained_inputs()
    k = synth.parse_model_table(cases.MODEL_CPG)[1]
    pm = sa.Model.load(cases.MODEL_CPG)
    maps = [dict(contig=0, x_sign=-1 if j == 2 else 1, x0=1000 * (j + 1) + (900 if j == 2 else 0), strand=j % 2,
                 mapped_strand=1 if j in (1, 2) else 0, true_letter=1 if j == 4 else -1) for j in range(len(jobs))]
    truth = [(m["contig"], m["x0"] + m["x_sign"] * x, m["mapped_strand"], "CE"[x % 2]) for job, m in zip(jobs, maps)
             for x in range(len(job["ref"]) - k + 1) if job["ref"][x + k - 1] == "X" and x % 5]
    scores = sa.CallScores("CE", truth=truth, n_bins=10, threshold=THRESHOLD)
    for flags in (0, sa.FLAG_EXACT):
        b = sa.Batch(pm, sa.default_params(), jobs, ambig=sa.default_ambig({"X": "CE"}), flags=flags | sa.FLAG_SITE_CALLS)
        b.run()
        mea = [m[0] for m in b.mea()]
        calls = b.site_calls()
        pairs = [b.pairs(j) for j in range(len(jobs))]
        first = lambda arrs: np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
        want = sa.call_quality_records(scores, maps, cq_jobs, first([c["x"] for c in calls]), np.concatenate([c["x"] for c in calls]),
                                       np.concatenate([c["prob"][:, :2] for c in calls]), first(pairs),
                                       np.concatenate([p["x"] for p in pairs]), np.concatenate([p["y"] for p in pairs]), mea=mea,
                                       flags=sa.CQ_CALLS)
        got = sa.batch_call_quality(scores, b, maps, cq_jobs, mea=mea, flags=sa.CQ_CALLS)
        keys = ("reads", "calls", "gaps", "hist", "total_hist")
        assert all(got[q].tobytes() == want[q].tobytes() for q in keys)
        r = got["reads"]
        assert r["n_calls"].sum() > 50 and r["n_unlabelled"].sum() > 5 and r["n_gaps"].sum() > 5 and r["n_correct"].sum() > 0
        assert int(r["status"][5]) & sa.CQ_NO_SITES and int(r["n_calls"][4]) > 0 and int(r["n_unlabelled"][4]) == 0
        assert got["total_hist"].sum() == (r["n_calls"] - r["n_outside"]).sum() > 20
        direct = sa.batch_call_quality(scores, b, maps, cq_jobs, mea=mea, flags=sa.CQ_CALLS | sa.CQ_BAND_DIRECT)
        assert all(direct[q].tobytes() == want[q].tobytes() for q in keys)
        # the accumulator is only read: finish gives the same rows with and without the call in between
        plain = sa.CallScores("CE", truth=truth, n_bins=10, threshold=THRESHOLD)
        plain.add_batch(b, maps)
        scores.checkpoint()
        scores.add_batch(b, maps)
        sa.batch_call_quality(scores, b, maps, cq_jobs, mea=mea)
        rows, curves, counts = scores.finish()
        rows0, curves0, counts0 = plain.finish()
        assert rows.tobytes() == rows0.tobytes() and curves.tobytes() == curves0.tobytes() and counts == counts0
        scores.rollback()
        plain.close()
        if flags == 0:
            # the batch refusals
            for change, code in ((dict(maps=maps[:-1], cq=cq_jobs[:-1], mea=mea[:-1]), SA_EINVAL),
                                 (dict(cq=[dict(c, raw_start=c["raw_start"][:-1], raw_length=c["raw_length"][:-1]) if q == 0 else c
                                            for q, c in enumerate(cq_jobs)]), SA_EINVAL)):
                with pytest.raises(sa.SaError) as e:
                    sa.batch_call_quality(scores, b, change.get("maps", maps), change.get("cq", cq_jobs), mea=change.get("mea", mea))
                assert e.value.code == code
            b.release_device()                                           # the pairs go up again
            after = sa.batch_call_quality(scores, b, maps, cq_jobs, mea=mea, flags=sa.CQ_CALLS)
            assert all(after[q].tobytes() == want[q].tobytes() for q in keys)
        b.close()
    no_flag = sa.Batch(pm, sa.default_params(), jobs[:2], ambig=sa.default_ambig({"X": "CE"}))
    no_flag.run()
    not_run = sa.Batch(pm, sa.default_params(), jobs[:2], ambig=sa.default_ambig({"X": "CE"}), flags=sa.FLAG_SITE_CALLS)
    for b in (no_flag, not_run):
        with pytest.raises(sa.SaError) as e:
            sa.batch_call_quality(scores, b, maps[:2], cq_jobs[:2])
        assert e.value.code == SA_ESTATE
        b.close()
    scores.close()
    sa.call_quality_release()
