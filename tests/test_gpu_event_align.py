"""Event <-> k-mer pre-alignment (adaptive_banded_simple_event_align, impl/eventAligner.c:899-1235): the HIP path
against the CPU restatement.  PARITY UNPINNED against the reference itself -- its tests of this function read fast5
files (tests/eventAlignerTests.c:223-320, :404-430) -- so what is checked here is: bit-identical pair lists and status
words between the two restatements, and properties any correct alignment has (monotone, spanning, every event between
the first and last aligned event used once, agreement with the generator's ground truth).  Behind the restatement
stands a plain full-matrix Viterbi, compared on the CPU on the shapes of tests/ea_cases.py
(tests/test_oracle_event_align.py); the same shapes are run here, with the cell count.
"""
import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import sa_cases as cases
import ea_cases

pytestmark = pytest.mark.gpu


def _jobs(oracle, model_path, n, n_events, first=0, noise=1.0):
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    om = oracle.Model(alpha, k, t10, tab)
    pm = sa.Model.load(model_path)
    jobs, truth = [], []
    for i in range(n):
        r = synth.make_read(first + i, n_events, alpha, k, tab)
        ev = np.ascontiguousarray(np.asarray(r["events4"])[:, 0])
        if noise != 1.0:
            rng = np.random.default_rng(i)
            ev = ev + rng.normal(0, noise, len(ev))
        seq = r["ref"]
        sh, sc = sa.scalings_mom(pm, seq, ev)
        osh, osc = oracle.scalings_mom(om, ev, oracle.kmer_ids_of(om, seq))
        assert sh == osh and sc == osc
        jobs.append(dict(sequence=seq, event_mean=ev, scale=sc, shift=sh, var=1.0))
        truth.append(r)
    return pm, om, jobs, truth


@pytest.mark.parametrize("model_path,n_events", [(cases.MODEL_6MER, 1500), (cases.MODEL_5MER, 600), (cases.MODEL_6MER, 40)])
def test_matches_the_cpu_restatement_bit_for_bit(oracle, model_path, n_events):
    pm, om, jobs, truth = _jobs(oracle, model_path, 6, n_events, first=77)
    got = sa.event_align_batch(pm, jobs)
    for j, job in enumerate(jobs):
        om.set_read_params(job["scale"], job["shift"], 1.0)
        ek, ee, est = oracle.event_align(om, job["event_mean"], oracle.kmer_ids_of(om, job["sequence"]))
        gk, ge, gst = got[j]
        assert gst == est, j
        assert np.array_equal(gk, ek) and np.array_equal(ge, ee), j


def test_alignment_properties_and_ground_truth(oracle):
    pm, om, jobs, truth = _jobs(oracle, cases.MODEL_6MER, 4, 3000, first=500)
    got = sa.event_align_batch(pm, jobs)
    for (gk, ge, st), job, r in zip(got, jobs, truth):
        assert st == 0 and len(gk) > 0
        n_kmers = len(job["sequence"]) - 5
        assert gk[0] == 0 and gk[-1] == n_kmers - 1                       # spanned
        dk, de = np.diff(gk), np.diff(ge)
        assert ((dk == 0) | (dk == 1)).all() and ((de == 0) | (de == 1)).all() and ((dk + de) >= 1).all()
        assert len(set(zip(gk.tolist(), ge.tolist()))) == len(gk)
        # the generator knows which k-mer produced every event: the Viterbi path finds it within one position almost always
        emap = np.asarray(r["event_map"])                                 # base -> first event
        owner = np.searchsorted(emap[:n_kmers], ge, side="right") - 1
        assert (np.abs(owner - gk) <= 1).mean() > 0.97


def test_rejected_alignment_reports_why(oracle):
    # events that have nothing to do with the sequence: the average emission check fires and the list comes back empty
    pm, om, jobs, truth = _jobs(oracle, cases.MODEL_6MER, 2, 800, first=900)
    rng = np.random.default_rng(5)
    jobs[0]["event_mean"] = rng.uniform(40, 140, len(jobs[0]["event_mean"]))
    got = sa.event_align_batch(pm, jobs)
    om.set_read_params(jobs[0]["scale"], jobs[0]["shift"], 1.0)
    ek, ee, est = oracle.event_align(om, jobs[0]["event_mean"], oracle.kmer_ids_of(om, jobs[0]["sequence"]))
    assert got[0][2] == est and est != 0 and len(got[0][0]) == 0 and len(ek) == 0
    assert got[1][2] == 0 and len(got[1][0]) > 0


def test_rna_kmer_list(oracle):
    # build_kmer_list(..., rna=true): U -> T, every k-mer reversed (impl/eventAligner.c:772-780)
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_5MER)
    om = oracle.Model(alpha, k, t10, tab)
    pm = sa.Model.load(cases.MODEL_5MER)
    r = synth.make_read(4242, 700, alpha, k, tab)
    seq = r["ref"].replace("T", "U")
    ids = oracle.kmer_ids_of(om, seq, rna=True)
    assert not np.array_equal(ids, oracle.kmer_ids_of(om, r["ref"]))
    # events drawn for the reversed k-mers, so that the alignment is accepted
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 3, size=len(ids))
    owner = np.repeat(np.arange(len(ids)), counts)
    ev = rng.normal(tab[5 * ids[owner]], tab[5 * ids[owner] + 1])
    sh, sc = sa.scalings_mom(pm, seq, ev, flags=sa.FLAG_RNA)
    assert (sh, sc) == oracle.scalings_mom(om, ev, ids)
    got = sa.event_align_batch(pm, [dict(sequence=seq, event_mean=ev, scale=sc, shift=sh, var=1.0)], flags=sa.FLAG_RNA)[0]
    om.set_read_params(sc, sh, 1.0)
    ek, ee, est = oracle.event_align(om, ev, ids)
    assert got[2] == est == 0 and np.array_equal(got[0], ek) and np.array_equal(got[1], ee)


def test_non_unit_variance_and_a_long_read(oracle):
    """var != 1 takes the kernel instance that keeps the division by var (the reference always passes 1, but the
    arithmetic is part of the emission); a 12000-event read crosses many refills of the event and k-mer stream buffers
    and many 64-band traceback blocks."""
    pm, om, jobs, truth = _jobs(oracle, cases.MODEL_6MER, 3, 2500, first=31)
    for j, v in zip(jobs, (1.3, 0.8, 1.0)):
        j["var"] = v
    long_pm, long_om, long_jobs, _ = _jobs(oracle, cases.MODEL_6MER, 1, 12000, first=5)
    jobs = jobs + long_jobs
    got = sa.event_align_batch(pm, jobs)
    for j, job in enumerate(jobs):
        om.set_read_params(job["scale"], job["shift"], job["var"])
        ek, ee, est = oracle.event_align(om, job["event_mean"], oracle.kmer_ids_of(om, job["sequence"]))
        gk, ge, gst = got[j]
        assert gst == est, j
        assert np.array_equal(gk, ek) and np.array_equal(ge, ee), j
    assert got[3][2] == 0 and len(got[3][0]) > 12000
    # all-unit batch again right after: the other kernel instance, same workspace
    again = sa.event_align_batch(pm, long_jobs)
    assert np.array_equal(again[0][0], got[3][0]) and np.array_equal(again[0][1], got[3][1])


def test_a_batch_equals_its_jobs_one_at_a_time_and_scratch_is_reused(oracle):
    """Release, a small call, the full call twice (the first grows every slot of the scratch, the second reuses it), every job
    alone, release, the full call again: the same pair lists and status words each time."""
    pm, jobs = None, []
    for i, n_events in enumerate((40, 400, 75, 260, 130, 333, 57, 190)):
        pm, _, one, _ = _jobs(oracle, cases.MODEL_6MER, 1, n_events, first=1300 + i)
        jobs += one

    def same(a, b):
        return len(a) == len(b) and all(x[2] == y[2] and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
                                        for x, y in zip(a, b))
    release = sa.lib().sa_event_align_release
    release()
    small = sa.event_align_batch(pm, jobs[:3])
    first = sa.event_align_batch(pm, jobs)
    second = sa.event_align_batch(pm, jobs)
    assert all(st == 0 and len(k) > 0 for k, _, st in first)
    assert same(first, second) and same(first[:3], small)
    assert same([sa.event_align_batch(pm, [j])[0] for j in jobs], first)
    release()
    assert same(sa.event_align_batch(pm, jobs), first)


# ---- the listed shapes (tests/ea_cases.py): the band, the two operand streams, the traceback blocks and the status
# thresholds at their edges, against sao_event_align_ex; tests/test_oracle_event_align.py stands behind the oracle there

_LISTS = {"6mer": (cases.MODEL_6MER, 0), "rna": (cases.MODEL_5MER, sa.FLAG_RNA)}


def _listed(which):
    """(model, flags, jobs, expected) of one list.  Nothing whose walk leaves the band on the oracle goes to the GPU:
    the kernel would index past its staged trace rows there."""
    model_path, flags = _LISTS[which]
    cs = ea_cases.cases_rna() if which == "rna" else ea_cases.cases_6mer()
    exp = ea_cases.expected(which)
    assert all(e[4] == 0 for e in exp), [c[0] for c, e in zip(cs, exp) if e[4]]
    jobs = [dict(sequence=seq, event_mean=ev, scale=sc, shift=sh, var=var) for _, seq, ev, sc, sh, var in cs]
    return sa.Model.load(model_path), flags, jobs, exp


def _assert_as_expected(got, cells, jobs, exp, what):
    assert len(got) == len(exp) == len(cells)
    for j, ((gk, ge, gst), (ek, ee, est, fills, _)) in enumerate(zip(got, exp)):
        where = (what, j, len(jobs[j]["event_mean"]), len(jobs[j]["sequence"]))
        assert gst == est, where
        assert np.array_equal(gk, ek) and np.array_equal(ge, ee), where
        assert cells[j] == fills, where + (cells[j], fills)


@pytest.mark.parametrize("which", ["6mer", "rna"])
def test_listed_shapes_in_one_call_pairs_status_and_cells(oracle, which):
    """One call per model and flag: status words, pair lists and the cell count (the numerator of bench.py's
    event_align_band_cell_updates_per_s) equal the oracle's, exactly.  The 6-mer list holds var != 1 beside var == 1."""
    pm, flags, jobs, exp = _listed(which)
    if which == "6mer":
        assert {j["var"] for j in jobs} >= {1.0, 1.3, 0.8}
        assert {e[2] for e in exp} >= {0, 1, 5, 8, 9}
    stats = {}
    got = sa.event_align_batch(pm, jobs, flags=flags, stats=stats)
    _assert_as_expected(got, stats["cells"], jobs, exp, which)


@pytest.mark.parametrize("which", ["6mer", "rna"])
def test_listed_shapes_one_job_per_call(oracle, which):
    """Every job alone: the per-read offsets into trace, ll, col and out (and the 4-byte alignment of the 100-byte trace
    rows the traceback loads as words) are all zero here and arbitrary in the batch; a var == 1 job alone takes the
    unit-variance instance of the kernel, in the 6-mer batch the other."""
    pm, flags, jobs, exp = _listed(which)
    got, cells = [], []
    for job in jobs:
        stats = {}
        got.append(sa.event_align_batch(pm, [job], flags=flags, stats=stats)[0])
        cells.append(stats["cells"][0])
    _assert_as_expected(got, cells, jobs, exp, which + " alone")


def test_listed_shapes_on_a_stale_and_on_a_fresh_trace_plane(oracle):
    """The trace plane is kept between calls and never cleared: after a 12000-event read every byte the short reads'
    tracebacks could reach holds another read's moves.  The list gives the same on that plane and on a fresh one."""
    pm, flags, jobs, exp = _listed("6mer")
    _, _, long_jobs, _ = _jobs(oracle, cases.MODEL_6MER, 1, 12000, first=5)
    release = sa.lib().sa_event_align_release
    release()
    long_got = sa.event_align_batch(pm, long_jobs)
    assert long_got[0][2] == 0 and len(long_got[0][0]) > 12000
    for what in ("stale plane", "fresh plane"):
        stats = {}
        got = sa.event_align_batch(pm, jobs, flags=flags, stats=stats)
        _assert_as_expected(got, stats["cells"], jobs, exp, what)
        release()


def test_a_value_that_is_not_finite_is_refused_before_the_kernel(oracle, capfd):
    """NaN event means make the reference's own traceback leave the band: sa_event_align_batch refuses the
    batch on the host -- SA_EINVAL and one line on stderr -- for an event mean, scale, shift or var that is not finite,
    whichever job of the batch holds it; the good read beside it aligns as before when sent again."""
    pm, flags, jobs, exp = _listed("6mer")
    at = next(j for j, c in enumerate(ea_cases.cases_6mer()) if c[0] == "matched_114k")
    good = jobs[at]

    def broken(**kw):
        bad = dict(good)
        for key, (idx, val) in kw.items():
            if idx is None:
                bad[key] = val
            else:
                arr = np.array(bad[key], dtype=np.float64)
                arr[idx] = val
                bad[key] = arr
        return bad
    bad_jobs = [broken(event_mean=(57, np.nan)), broken(event_mean=(len(good["event_mean"]) - 1, np.inf)),
                broken(event_mean=(0, -np.inf)), broken(scale=(None, np.nan)), broken(shift=(None, np.inf)),
                broken(var=(None, np.inf))]
    for i, bad in enumerate(bad_jobs):
        capfd.readouterr()
        with pytest.raises(sa.SaError) as ei:
            sa.event_align_batch(pm, [good, bad] if i % 2 else [bad, good])
        err = capfd.readouterr().err
        assert ei.value.code == -1 and "not a finite number" in err and err.count("\n") == 1, (i, err)
        stats = {}
        again = sa.event_align_batch(pm, [good], stats=stats)
        _assert_as_expected(again, stats["cells"], [good], [exp[at]], "after refusal %d" % i)
