"""Shared inputs of tests/test_oracle_outlier_events.py and tests/test_gpu_outlier_events.py: reads whose events do NOT fit the
model that aligns them -- means in a tail of their emission or beyond the HDP's grid, noise that is tiny, huge or zero -- and the
CPU oracle's answer for each, computed once per process.

Every other alignment test draws its events from the model under test (synth.make_read, cases.events_for_sequence,
synth.make_read_hdp).  Here a seeded read is drawn the same way and then a few of its events are overwritten.  A job made here is
the usual dict with three more keys: "label" (read, place, change), "outliers" (indices of the changed events) and "kind" (what
the oracle makes of it: see the suites below).  Only data is made here; none of the aligner's arithmetic.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from signalalign_amd import synth

import sa_cases as cases

WHERE = ("first", "last", "every37", "run3", "seg_edge")
SPLIT_SMALL = 250 * 250
TRACE_BACK, MIN_DIAGS, EXPANSION = 100, 1000, 50      # the default parameters (sa.default_params / oracle.default_params)


def _oracle():
    from oracle import sa_oracle_py
    sa_oracle_py.lib()
    return sa_oracle_py


def seg_edge_event(job, k, expansion=EXPANSION, trace_back=TRACE_BACK, min_diags=MIN_DIAGS):
    """The event nearest the first diagonal of the second traceback segment of the job's (unsplit) matrix, or None when the matrix
    has one traceback only.  The walk is getPosteriorProbsWithBanding's (impl/pairwiseAligner.c:1450-1590): the first diagonal
    d >= min_diags whose band is no wider than 2 expansion + 1 cells starts a traceback that hands out posteriors up to diagonal
    d - trace_back - 1; the next segment begins one further."""
    lX, lY = len(job["ref"]) - (k - 1), len(job["events"])
    L, R = _oracle().band(job["ax"], job["ay"], lX, lY, expansion)
    for d in range(min_diags, lX + lY):
        if (R[d] - L[d]) // 2 + 1 <= 2 * expansion + 1:
            e = d - trace_back
            y = (e - (int(L[e]) + int(R[e])) // 2) // 2          # matrix row of the band's middle cell on that diagonal
            return int(min(max(y - 1, 0), lY - 1))
    return None


def where_events(job, where, k):
    """indices of the events a place name stands for; an empty array where the read has no such place (seg_edge in a short read)"""
    n = len(job["events"])
    if where == "first":
        return np.array([0])
    if where == "last":
        return np.array([n - 1])
    if where == "every37":
        return np.arange(7, n, 37)
    if where == "run3":
        return np.arange(n // 2 - 1, n // 2 + 2)
    if where == "run70":
        return np.arange(n // 2, n // 2 + 70)
    if where == "seg_edge":
        e = seg_edge_event(job, k)
        return np.array([e] if e is not None else [], dtype=np.int64)
    if isinstance(where, str) and where.startswith("every"):
        return np.arange(7, n, int(where[5:]))
    return np.asarray(where, dtype=np.int64)                      # explicit indices


def _changed(job, idx, label):
    q = dict(job)
    q["events"] = np.array(job["events"], dtype=np.float64, copy=True)
    q["outliers"] = np.asarray(idx, dtype=np.int64)
    q["label"] = "%s %s" % (job.get("label", "read"), label)
    return q


def with_outlier_means(job, where, delta, k=6):
    """a copy of the job with `delta` added to the mean of the events at `where`"""
    idx = where_events(job, where, k)
    q = _changed(job, idx, "mean%+g@%s" % (delta, where))
    q["events"][idx, 0] += delta
    return q


def with_noise(job, where, factor=None, value=None, k=6):
    """a copy of the job with the noise of the events at `where` multiplied by `factor` or set to `value`"""
    idx = where_events(job, where, k)
    q = _changed(job, idx, ("noise*%g@%s" % (factor, where)) if value is None else ("noise=%r@%s" % (value, where)))
    if value is None:
        q["events"][idx, 1] *= factor
    else:
        q["events"][idx, 1] = value
    return q


# what hdp_grid_end_events writes, as (name, event as a function of the grid's two ends, density is positive there).  The zone with
# a positive density beyond the last grid point of the bundled model is about 6 wide (its density falls linearly from 1.1e-3).
GRID_END = (("g0", lambda a, b: a, True), ("g0-ulp", lambda a, b: np.nextafter(a, -np.inf), True),
            ("g0+ulp", lambda a, b: np.nextafter(a, np.inf), True), ("g0-5", lambda a, b: a - 5.0, True),
            ("g0-50", lambda a, b: a - 50.0, False),
            ("gN", lambda a, b: b, True), ("gN-ulp", lambda a, b: np.nextafter(b, -np.inf), True),
            ("gN+ulp", lambda a, b: np.nextafter(b, np.inf), True), ("gN+0.5", lambda a, b: b + 0.5, True),
            ("gN+5", lambda a, b: b + 5.0, True), ("gN+50", lambda a, b: b + 50.0, False))


def hdp_grid_end_events(job, grid, names, at):
    """A copy of a job with scale = var = 1, shift = 0 (the standardised event IS the event) whose events at[i] hold the grid-end
    value names[i] (see GRID_END).  at: event indices, or a place name for a single value written to every event of the place."""
    assert job["scale"] == 1.0 and job["var"] == 1.0 and job["shift"] == 0.0
    g0, gN = float(grid[0]), float(grid[-1])
    fn = {n: f for n, f, _ in GRID_END}
    if isinstance(at, str):
        idx = where_events(job, at, 6)
        vals = np.full(len(idx), fn[names[0]](g0, gN))
        label = "%s@%s" % (names[0], at)
    else:
        idx = np.asarray(at, dtype=np.int64)
        vals = np.array([fn[n](g0, gN) for n in names])
        label = "grid ends " + ",".join(names)
    q = _changed(job, idx, label)
    q["events"][idx, 0] = vals
    return q


def _no_anchors(job):
    return dict(job, ax=np.zeros(0, dtype=np.int64), ay=np.zeros(0, dtype=np.int64))


def _labelled(job, label):
    return dict(job, label=label, outliers=np.zeros(0, dtype=np.int64))


def gaussian_reads(model_path, first_index=5):
    """The unmodified reads of one ACGT model: (a) dense anchors, 60 / 400 / 1700 events (register kernels; 1700 events are three
    tracebacks under default parameters), (b) 1500 events with the anchors of a real guide alignment (ring kernels; with
    SA_RING_WIDE=0 the register kernels' wide path), (c) 900 events with thinned anchors and 260 events without any (strip kernels)."""
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    reads = [_labelled(synth.make_read(first_index + i, n, alpha, k, tab), "a%d" % n) for i, n in enumerate((60, 400, 1700))]
    reads.append(_labelled(cases.realistic_anchor_jobs(model_path, 1, 1500, first_index + 10)[0], "b1500"))
    reads.append(_labelled(synth.make_read(first_index + 20, 900, alpha, k, tab, thin_anchors=0.35), "c900"))
    reads.append(_labelled(_no_anchors(synth.make_read(first_index + 21, 260, alpha, k, tab)), "c260"))
    return reads, k


def cpg_reads(first_index=40):
    """(d): 1100 events, every CpG cytosine / every 20th an ambiguity letter: the dense and the sparse multi-path ring instance"""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    return [_labelled(synth.make_read(first_index + i, 1100, alpha, k, tab, cpg_ambiguous=True, cpg_every=every), "d1100/%d" % every)
            for i, every in enumerate((1, 20))], k


def variants(reads, k, changes, wheres=WHERE):
    """reads + every (read, place, change) copy; changes: functions (job, where, k) -> job.  A read without the place is skipped."""
    out = list(reads)
    for r in reads:
        for where in wheres:
            if len(where_events(r, where, k)) == 0:
                continue
            for ch in changes:
                out.append(ch(r, where, k))
    return out


def mean_shifts(*deltas):
    return [lambda job, where, k, d=d: with_outlier_means(job, where, d, k) for d in deltas]


def r73_reads(table5=None, first_index=5):
    """The HDP reads: R7.3 synth.make_read reads of 400 and 1700 events (dense anchors, register kernels), the 400-event read with
    three-way and two-way ambiguity codes (L, P: ring kernels through k_emit_hdp_ring), a 900-event read with the anchors of a real
    guide alignment (strip kernels) and two reads drawn from the HDP's own densities (cases.hdp_jobs)."""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_R73)
    reads = [_labelled(synth.make_read(first_index, n, alpha, k, tab), "h%d" % n) for n in (400, 1700)]
    ref = list(reads[0]["ref"])
    for i in range(7, len(ref) - 6, 23):
        ref[i] = "L" if (i // 23) % 2 == 0 else "P"
    reads.append(_labelled(dict(reads[0], ref="".join(ref)), "h400LP"))
    thin = cases.thin_anchors_like_a_guide_alignment([synth.make_read(first_index + 1, 900, alpha, k, tab)])[0]
    reads.append(_labelled(thin, "h900thin"))
    # (46 305 of the bundled model's 46 656 k-mers share the base process's density: on a random reference an event's emission is
    # the same for every k-mer of its row and cancels out of the posteriors.  These two references come from the sequence the model
    # was trained on, whose k-mers have densities of their own -- with their own values and slopes at the grid's ends)
    reads.append(_labelled(cases.hdp_jobs(1, 400, first_index + 2, table5=table5)[0], "hdp400"))
    reads.append(_labelled(cases.hdp_jobs(1, 1700, first_index + 3, table5=table5)[0], "hdp1700"))
    return reads, k


# ---- the oracle's answers, once per process ------------------------------------------------------------------------------------
_EXPECTED = {}


def oracle_rows(key, make_model, jobs, params, ambig=None):
    """[(pairs, Stats)] of the CPU oracle for `jobs`, cached under `key`.  make_model(): a fresh oracle Model -- one per worker
    thread, because a job's scaling is set on the model (set_read_params) before it is aligned."""
    if key in _EXPECTED:
        return _EXPECTED[key]
    oracle = _oracle()
    n_threads = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
    chunks = [list(range(t, len(jobs), n_threads)) for t in range(n_threads)]

    def work(ids):
        om = make_model()
        out = []
        for i in ids:
            job = jobs[i]
            om.set_read_params(job["scale"], job["shift"], job["var"])
            out.append((i, oracle.align(om, job["ref"], job["events"], job["ax"], job["ay"], params, ambig=ambig,
                                        ragged=job.get("ragged", (1, 1)), want_stats=True)))
        return out
    res = [None] * len(jobs)
    with ThreadPoolExecutor(n_threads) as ex:
        for part in ex.map(work, chunks):
            for i, r in part:
                res[i] = r
    _EXPECTED[key] = res
    return res


def regions_of(job, k, split):
    """(y1, y2) event ranges of the rectangles the reference splits the job's matrix into (sao_split_points)"""
    lX, lY = len(job["ref"]) - (k - 1), len(job["events"])
    rl, rr = job.get("ragged", (1, 1))
    sp = _oracle().split_points(job["ax"], job["ay"], lX, lY, split, rl, rr)
    return [(int(r[1]), int(r[3])) for r in sp]


# ---- the suites: one list of jobs per model, every job with its "kind" ------------------------------------------------------------
# "tail":   means moved into a tail of the emission; the oracle's total stays finite and |total| < 1e8 (the CPU test pins it), so the
#           1e-5 bar of the default kernels applies
# "far":    |total| >= 1e8: the reference itself has lost the digits a posterior needs; only what does not depend on them is asserted
# "neginf": an emission of -inf in every path: total -inf, no rows from any traceback that reaches the event
NEGINF_WHERE = ("first", "last", "run3", "seg_edge")


def _kind(jobs, kind):
    return [dict(j, kind=kind) for j in jobs]


def gaussian_suite(model_path):
    """(jobs, k, n_reads) for an ACGT Gaussian model: the reads of gaussian_reads, then their variants"""
    reads, k = gaussian_reads(model_path)
    n = len(reads)
    jobs = _kind(reads, "tail")
    jobs += _kind(variants(reads, k, mean_shifts(30.0, -30.0, 200.0, -200.0, 1e4))[n:], "tail")
    jobs += _kind(variants(reads, k, mean_shifts(1e6))[n:], "far")
    jobs += _kind(variants(reads, k, mean_shifts(1e300), wheres=NEGINF_WHERE)[n:], "neginf")
    return jobs, k, n


def cpg_suite():
    reads, k = cpg_reads()
    return _kind(variants(reads, k, mean_shifts(30.0, -30.0, 200.0, -200.0)), "tail"), k, len(reads)


def hdp_suite(table5, grid):
    """R7.3 reads under the bundled HDP: +-30 shifts (inside the grid or in the zone beyond it where the density is still positive:
    tails), every grid-end value with a positive density -- one among interior events (a wave that takes the extrapolation branch for
    one lane while the others keep their cubic), the first two events (diagonals 1 and 2 hold nothing else) and a run of 70 (whole
    diagonals of a wide band) -- and the values without a density, +200 included: -inf rows."""
    reads, k = r73_reads(table5)
    n = len(reads)
    shifted = [r for r in reads if not r["label"].startswith("hdp")]
    own = [r for r in reads if r["label"].startswith("hdp")]     # (their events reach 94: +30 would leave the zone with a density)
    jobs = _kind(reads, "tail")
    jobs += _kind(variants(shifted, k, mean_shifts(30.0, -30.0))[len(shifted):], "tail")
    jobs += _kind(variants(own, k, mean_shifts(-30.0), wheres=("first", "last", "every37"))[len(own):], "tail")
    for r in reads:
        ident = identity_scaled(r)
        ne = len(r["events"])
        pos = [nm for nm, _, positive in GRID_END if positive]
        scattered = 11 + 29 * np.arange(len(pos))               # one off-interior event among interior ones, tile after tile
        if scattered[-1] < ne:
            jobs.append(dict(hdp_grid_end_events(ident, grid, pos, scattered), kind="tail"))
        jobs.append(dict(hdp_grid_end_events(ident, grid, ["gN+0.5", "g0-5", "gN+5"], [0, 1, ne - 1]), kind="tail"))
        if ne > 1000:
            for nm in ("gN+0.5", "g0-5"):
                jobs.append(dict(hdp_grid_end_events(ident, grid, [nm], "run70"), kind="tail"))
        jobs.append(dict(ident, kind="tail", label=r["label"] + " identity"))
        for where in NEGINF_WHERE:
            if len(where_events(r, where, k)) == 0:
                continue
            for nm in ("gN+50", "g0-50"):
                jobs.append(dict(hdp_grid_end_events(ident, grid, [nm], where), kind="neginf"))
            jobs.append(dict(with_outlier_means(r, where, 200.0, k), kind="neginf"))
    return jobs, k, n


NOISE_FACTORS = (1e-3, 1e-6, 30.0, 1e3)
NOISE_WHERE = ("every37", "first", "last")


def two_dist_suite(emission):
    """Reads of the CpG model (it holds every ACGT k-mer too) for the two-distribution emissions: a register, a strip and two ring
    reads as in test_gpu_two_dist_kernels.test_noise_scaling_per_read, and their copies with the noise of some events scaled (tails),
    set to 1e300 (-inf rows) or, under SA_EMISSION_TWO_DIST (1) only, set to zero (the 1e-9 replacement: |total| about 8e9, a far tail).
    emission 2 takes the event as it is: identity scaling."""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    reads = [_labelled(synth.make_read(300, 400, alpha, k, tab), "reg400"),
             _labelled(cases.realistic_anchor_jobs(cases.MODEL_CPG, 1, 1500, 600)[0], "strip1500")]
    reads += cpg_reads()[0]
    if emission == 2:
        reads = [identity_scaled(r) for r in reads]
    n = len(reads)
    jobs = _kind(reads, "tail")
    scale = [lambda job, where, k, f=f: with_noise(job, where, factor=f, k=k) for f in NOISE_FACTORS]
    jobs += _kind(variants(reads, k, scale, wheres=NOISE_WHERE)[n:], "tail")
    if emission == 1:
        jobs += _kind(variants(reads, k, [lambda job, where, k: with_noise(job, where, value=0.0, k=k)], wheres=NOISE_WHERE)[n:], "far")
    jobs += _kind(variants(reads, k, [lambda job, where, k: with_noise(job, where, value=1e300, k=k)], wheres=NEGINF_WHERE)[n:], "neginf")
    return jobs, k, n


def identity_scaled(job):
    """the job with scale = var = 1, shift = 0 and its event means moved to where the model expects them under that scaling"""
    q = dict(job, scale=1.0, shift=0.0, var=1.0)
    q["events"] = np.array(job["events"], dtype=np.float64, copy=True)
    q["events"][:, 0] = (q["events"][:, 0] - job["shift"]) / job["scale"]
    return q
