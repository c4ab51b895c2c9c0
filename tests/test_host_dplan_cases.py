"""tests/dplan_cases.py on the host, no GPU: every case the device planner must take is a job the host planner accepts as one
region whose band is the oracle's and whose traceback segments follow the schedule's rule, restated below; the cases it must
decline are declined for the reason their name gives; and the facts the cases were built for (a segment with more than 256
checkpoints, reads on both kinds of kernel on either side of a tile, a forward-storage pass that ends at the tile, the exact
anchor counts, the 50 x 50 rectangle) hold in the host plan before anything runs on a GPU.  The size of the table is fixed here:
a case cannot pass tests/test_gpu_dplan_edges.py by being declined."""
import numpy as np
import pytest

import signalalign_amd as sa

import dplan_cases as dc
import sa_cases as cases

_MODELS = {}


def _model(key):
    if key not in _MODELS:
        path, nhdp = dc.MODELS[key]
        _MODELS[key] = sa.Model.load(path, nhdp) if nhdp else sa.Model.load(path)
    return _MODELS[key]


def _ambig(case):
    return sa.default_ambig(case.ambig) if case.ambig else None


def check_schedule(segs, widths, N, p):
    """getPosteriorProbsWithBanding (impl/pairwiseAligner.c:1486-1518), the schedule only: a traceback starts on the first diagonal
    d >= tracedBackTo + minDiagsBetweenTraceBack whose band is at most 2 * expansion + 1 cells wide, or on the last diagonal N; it emits
    the diagonals (tracedBackTo, from] with from = d - (traceBackDiagonals + 1), from = N at the end; the next one starts from there."""
    tb, md, wlimit = p.trace_back_diagonals, p.min_diags_between_trace_back, 2 * p.diagonal_expansion + 1
    to, exp = 0, []
    while True:
        d = next((q for q in range(max(to + md, 1), N) if widths[q] <= wlimit), N)
        frm = N if d == N else d - (tb + 1)
        exp.append((0, d, frm, to))
        to = frm
        if d == N:
            break
    assert [tuple(int(v) for v in s) for s in segs] == exp
    return exp


def test_the_size_of_the_case_table():
    taken = [c.name for c in dc.CASES.values() if c.expect == 0]
    declined = sorted(c.name for c in dc.CASES.values() if c.expect == dc.NOT_TAKEN)
    assert len(taken) + len(declined) == len(dc.CASES)
    assert declined == ["g5_1025_bad_read_1024", "g6_behind_50x51", "g6_between_50x51", "g6_front_50x51"]
    assert len(taken) == 25 + 9 * 6 and len(dc.G7_BASES) == 9
    assert set(dc.ALIGNED) <= set(taken) and sorted(set(dc.CASES[n].group for n in dc.ALIGNED)) == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("name", [c.name for c in dc.CASES.values() if c.expect == 0])
def test_host_planner_takes_the_case_as_the_oracle_does(oracle, name):
    case = dc.CASES[name]
    m, k = _model(case.model), dc.kmer_length(case.model)
    p = sa.default_params(**dict(case.params))
    for j, job in enumerate(dc.jobs_of(case)):
        lX, lY = dc.dims(job, k)
        info, regions, rows, segs = cases.check_plan_geometry(oracle, sa, m, k, p, job, tag=(name, j), ambig=_ambig(case), flags=case.flags)
        assert regions.tolist() == [[0, 0, lX, lY]], (name, j)          # not split: one region, the whole matrix
        assert len(rows) == lX + lY + 1
        widths = (rows[:, 2] - rows[:, 1]) // 2 + 1
        assert len(check_schedule(segs, widths, lX + lY, p)) == info.n_segments, (name, j)


def _describe(name, j=0):
    case = dc.CASES[name]
    job = dc.jobs_of(case)[j]
    return job, sa.plan_describe(_model(case.model), sa.default_params(**dict(case.params)), job, ambig=_ambig(case), flags=case.flags)


def test_group1_diagonal_counts():
    for model in ("6mer", "5mer"):
        k = dc.kmer_length(model)
        d = [dc.dims(j, k) for j in dc.g1_jobs(model)]
        assert [lX + lY + 1 for lX, lY in d[:7]] == [255, 256, 257, 511, 512, 513, 769]
        assert d[7:] == [(255, 300), (256, 300), (257, 300)]
        assert all(len(j["ax"]) > 0.5 * dc.dims(j, k)[0] for j in dc.g1_jobs(model))        # dense anchors


def test_group2_paths_on_both_sides_of_the_scan_steps():
    jobs = dc.g2_jobs()
    k = dc.kmer_length("cpg")
    paths = []
    for j in jobs:
        lX = dc.dims(j, k)[0]
        paths.append([2 ** j["ref"][x - 1:x - 1 + k].count("X") for x in range(1, lX + 1)])   # cell x: paths[x - 1]
    assert [len(q) for q in paths[:12]] == [255] * 3 + [256] * 3 + [257] * 3 + [513] * 3
    # cells 256 | 257: 4, 2 and 1 paths on both sides; cells 512 | 513 of the reads that have them: 1, 4 and 2
    assert [(q[255], q[256]) for q in paths[6:12]] == [(4, 4), (2, 2), (1, 1)] * 2
    assert [(q[511], q[512]) for q in paths[9:12]] == [(1, 1), (4, 4), (2, 2)]
    assert [q[254] for q in paths[0:3]] == [4, 2, 1] and [q[255] for q in paths[3:6]] == [4, 2, 1]
    assert jobs[12]["ref"].index("X") == 0 and jobs[12]["ref"].count("X") == 1
    assert jobs[13]["ref"].index("X") == len(jobs[13]["ref"]) - 1
    info = sa.plan_digest(_model("cpg"), sa.default_params(), jobs, ambig=sa.default_ambig(dc.G2_AMBIG))[0]
    assert info.n_ring_regions == info.n_regions == len(jobs) == 14                         # the kernels with per-path records


def test_group3_anchor_lists():
    k = dc.kmer_length("6mer")
    jobs = dc.g3_lists("6mer")
    assert [len(j["ax"]) for j in jobs[:3]] == [0, 1, 2]
    assert (jobs[3]["ax"][0], jobs[3]["ay"][0]) == (0, 0)
    lX, lY = dc.dims(jobs[4], k)
    assert (jobs[4]["ax"][-1], jobs[4]["ay"][-1]) == (lX - 1, lY - 1)
    run = jobs[5]
    assert np.array_equal(run["ax"], np.arange(dc.G3_RUN)) and np.array_equal(run["ay"], run["ax"])
    assert dc.dims(run, k) == (dc.G3_RUN + dc.G3_STRETCH,) * 2
    rows = sa.plan_describe(_model("6mer"), sa.default_params(), run)[2]
    widest = int(((rows[:, 2] - rows[:, 1]) // 2 + 1).max())
    assert dc.G3_STRETCH <= widest <= 512
    for j in jobs:
        assert np.all(np.diff(j["ax"]) > 0) and np.all(np.diff(j["ay"]) > 0)
    big = dc.jobs_of(dc.CASES["g3_8191_8192_8193"])
    assert [len(j["ax"]) for j in big] == [8191, 8192, 8193] and [dc.dims(j, k) for j in big] == [(n + 7, n + 7) for n in dc.G3_BIG]
    alone = dc.jobs_of(dc.CASES["g3_8193_alone"])
    assert len(alone) == 1 and len(alone[0]["ax"]) == 8193 == len(alone[0]["ay"])
    own = dc.g3_big_own_anchors()[0]
    steps = np.diff(own["ay"])
    assert len(own["ax"]) == 8193 and np.all(np.diff(own["ax"]) > 0) and steps.min() >= 1 and steps.max() >= 4    # no straight line


def test_group4_schedule_shapes():
    k = dc.kmer_length("6mer")
    assert [len(j["events"]) for j in dc.g4_reads("6mer", *dc.G4_EVENTS)] == [400, 1000, 1001, 1100, 4000]
    assert [sum(dc.dims(j, k)) for j in dc.g4_on_min_diags("6mer")] == [299, 300, 301, 302]
    # one segment per diagonal, nearly: min_diags - trace_back - 1 = 1
    for name in ("g4_tb0_md2", "g4_tb1_md3", "g4_tb100_md102"):
        job, (info, regions, rows, segs) = _describe(name)
        assert info.n_segments > 0.8 * sum(dc.dims(job, k)) - 102 and len(segs) == info.n_segments
    for kw in (dict(trace_back=-1, min_diags=2), dict(trace_back=0, min_diags=1), dict(trace_back=1, min_diags=2)):   # still refused
        with pytest.raises(sa.SaError) as ei:
            sa.plan_describe(_model("6mer"), sa.default_params(**kw), dc.g4_reads("6mer", 400)[0])
        assert ei.value.code == -1, kw


@pytest.mark.parametrize("name", ["g4_tb0_md2", "g4_tb1_md3"])
def test_group4_shortest_tracebacks_do_the_oracles_work(oracle, name):
    """trace_back = 0 is a case the reference's debug build asserts against (impl/pairwiseAligner.c:1460) and its release build computes;
    the oracle computes it, and the plan announces the tracebacks and the cells the oracle's run performs."""
    case = dc.CASES[name]
    job = dc.jobs_of(case)[0]
    p = sa.default_params(**dict(case.params))
    info = sa.plan_describe(_model(case.model), p, job)[0]
    alpha, k, t10, tab = dc._table(case.model)
    om = oracle.Model(alpha, k, t10, tab)
    om.set_read_params(job["scale"], job["shift"], job["var"])
    _, st = oracle.align(om, job["ref"], job["events"], job["ax"], job["ay"], cases.oracle_params(oracle, p), want_stats=True)
    assert info.n_segments == st.n_tracebacks
    assert info.cells_forward == st.cells_forward and info.cells_backward == st.cells_backward
    # more checkpoints in one segment than the device planner has threads: a total-probability checkpoint every 10 diagonals
    job, (info, regions, rows, segs) = _describe("g4_tb100_md3000")
    assert max(int(s[2] - s[3]) for s in segs) > 2560


def test_group5_batches():
    m, p = _model("6mer"), sa.default_params()
    for n in dc.G5_SIZES:
        jobs = dc.jobs_of(dc.CASES["g5_%d" % n])
        assert len(jobs) == n
        info = sa.plan_digest(m, p, jobs)[0]
        assert info.n_regions == n
        if n in (1025, 2049):   # both kinds in front of the tile's end and behind it
            assert info.n_fast_regions > 0 and info.n_ring_regions > 0
            head = sa.plan_digest(m, p, jobs[:1024])[0]
            assert 0 < head.n_ring_regions <= info.n_ring_regions and 0 < head.n_fast_regions <= info.n_fast_regions
            assert head.n_ring_regions + head.n_fast_regions == 1024 and info.n_ring_regions + info.n_fast_regions == n
        else:
            assert all(3 <= len(j["events"]) <= 40 for j in jobs)
    # the forward-storage passes of the 2049-read batch: sa_plan_repack's greedy packing of the host plan's cell-paths per read
    case = dc.CASES["g5_2049_passes"]
    assert dict(case.env) == {"SA_F_BUDGET_CELLPATHS": "125000"}
    budget, used, chunk, chunk_of = 125000, 0, 0, []
    for job in dc.jobs_of(case):
        f = sa.plan_describe(m, p, job)[0].f_cellpaths
        if used > 0 and used + f > budget:
            chunk, used = chunk + 1, 0
        chunk_of.append(chunk)
        used += f
    assert chunk + 1 >= 40
    assert chunk_of[1025] == chunk_of[1023] + 1
    # the batch that is declined: read 1024, the first of the second tile, has a letter outside the alphabet
    bad = dc.jobs_of(dc.CASES["g5_1025_bad_read_1024"])
    assert len(bad) == 1025 and "N" in bad[1024]["ref"] and not any("N" in j["ref"] for j in bad[:1024])
    with pytest.raises(sa.SaError) as ei:
        sa.plan_describe(m, p, bad[1024])
    assert ei.value.code == -4                                     # SA_EALPHABET


def test_group6_the_rectangle_that_splits(oracle):
    k = dc.kmer_length("6mer")
    p = sa.default_params(split=dc.G6_SPLIT)
    for place in ("front", "between", "behind"):
        for gy, whole in ((50, True), (51, False)):
            job = dc.g6_job(place, gy)[0]
            lX, lY = dc.dims(job, k)
            ax, ay = job["ax"], job["ay"]
            px = np.concatenate([[0], ax + 1])
            py = np.concatenate([[0], ay + 1])
            gaps = (np.concatenate([ax, [lX]]) - px) * (np.concatenate([ay, [lY]]) - py)     # anchor-free rectangles
            assert int(gaps.max()) == 50 * gy and int((gaps > 0).sum()) == 1, (place, gy)
            regions = oracle.split_points(ax, ay, lX, lY, p.split_matrix_bigger_than_this, 1, 1).tolist()
            assert (regions == [[0, 0, lX, lY]]) == whole, (place, gy, regions)
