"""Site calls scored against known truth on the GPU (sa_call_scores_*): the rows of finish equal the restatement in Python integers
(call_scores_ref.py) fed from the batch's own site calls -- counts and auc2 exactly, auc bit for bit -- with positions truth and with
read-level labels, on host-finalised pairs and after the device storage went back; scores added as records; checkpoint and
rollback; the counts of dropped calls; the error contract."""
import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import call_scores_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

CE = {"X": "CE"}
N_BINS, THRESHOLD = 20, 0.500000001


def cpg_jobs():
    """the batch of test_gpu_site_calls.py: eight reads, one without any site, one with anchors as sparse as a guide alignment's"""
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 3, 1200, 40, cpg_ambiguous=True)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 3, 1200, 50, cpg_ambiguous=True, cpg_every=3)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 1, 900, 60)
    jobs += cases.thin_anchors_like_a_guide_alignment(cases.synthetic_jobs(cases.MODEL_CPG, 1, 1500, 70, cpg_ambiguous=True, cpg_every=3))
    assert sum("X" in j["ref"] for j in jobs) == len(jobs) - 1
    return jobs


def job_map(n_jobs, labelled=()):
    """reads 1 and 2 map to '-', read 2 runs against its reference_index; the strands alternate; two contigs"""
    out = []
    for j in range(n_jobs):
        sign = -1 if j == 2 else 1
        out.append(dict(contig=j % 2, x_sign=sign, x0=100000 * (j + 1) + (5000 if sign < 0 else 0), strand=j % 2,
                        mapped_strand=1 if j in (1, 2) else 0, true_letter=j % 2 if j in labelled else -1))
    return out


def positions_truth(jobs, maps, k, skip=7):
    """a positions table over every site of every job, change_to alternating by position; positions that are a multiple of `skip` are
    left out, and some keys are named twice with the other letter (the first line wins)"""
    lines = []
    for job, m in zip(jobs, maps):
        for x in range(len(job["ref"]) - k + 1):
            if job["ref"][x + k - 1] != "X":
                continue
            r = m["x0"] + m["x_sign"] * x
            if r % skip:
                lines.append((m["contig"], r, m["mapped_strand"], "CE"[r % 2]))
    lines += [(c, r, s, "CE"[1 - r % 2]) for c, r, s, _ in lines[::5]]
    table = {}
    for c, r, s, letter in lines:
        table.setdefault((c, r, s), letter)
    return lines, table


@pytest.fixture(scope="module")
def batches():
    alpha, k, _, _ = synth.parse_model_table(cases.MODEL_CPG)
    pm = sa.Model.load(cases.MODEL_CPG)
    jobs = cpg_jobs()
    made = {}

    def get(flags):
        if flags not in made:
            b = sa.Batch(pm, sa.default_params(), jobs, ambig=sa.default_ambig(CE), flags=flags | sa.FLAG_SITE_CALLS)
            b.run()
            made[flags] = (b, b.site_calls())
        return made[flags]

    yield jobs, k, get
    for b, _ in made.values():
        b.close()


def _finish(acc):
    rows, curves, counts = acc.finish()
    return rows, curves, counts


@pytest.mark.parametrize("flags", [0, sa.FLAG_EXACT])
def test_positions_truth_equals_the_restatement(batches, flags):
    jobs, k, get = batches
    b, calls = get(flags)
    maps = job_map(len(jobs))
    lines, table = positions_truth(jobs, maps, k)
    exp = ref.Scores("CE", N_BINS, THRESHOLD)
    exp.add_site_calls(calls, maps, table)
    rows = exp.rows()
    assert len(rows) == 6 and all(r["level"] == 0 and r["n_pos"] > 0 and r["n_neg"] > 0 for r in rows)
    assert exp.unlabelled > 5 and sum(r["n_pos"] + r["n_neg"] for r in rows[4:]) > 200
    acc = sa.CallScores("CE", truth=lines, n_bins=N_BINS, threshold=THRESHOLD)
    st = {}
    acc.add_batch(b, maps, stats=st)
    assert st["kernel_ms"] > 0
    got_rows, got_curves, counts = _finish(acc)
    ref.check_rows(got_rows, got_curves, rows)
    assert counts == dict(unlabelled=exp.unlabelled, other_sites=0)
    again = acc.finish()                                         # finish leaves the accumulator as it is
    assert again[0].tobytes() == got_rows.tobytes() and again[1].tobytes() == got_curves.tobytes()
    acc.close()
    if flags == 0:                                               # after the working storage went back (the pairs go up again)
        b.release_device()
        acc = sa.CallScores("CE", truth=lines, n_bins=N_BINS, threshold=THRESHOLD)
        acc.add_batch(b, maps)
        after = acc.finish()
        assert after[0].tobytes() == got_rows.tobytes() and after[1].tobytes() == got_curves.tobytes()
        acc.close()


def test_read_level_labels(batches):
    jobs, k, get = batches
    b, calls = get(sa.FLAG_EXACT)
    maps = job_map(len(jobs), labelled=(1, 2, 4, 6))            # half of the reads; 1 and 2 map to '-', 6 has no site
    lines, table = positions_truth(jobs, maps, k)
    exp = ref.Scores("CE", N_BINS, THRESHOLD)
    exp.add_site_calls(calls, maps, table)
    rows = exp.rows()
    level1 = [r for r in rows if r["level"] == 1]
    assert sum(r["n_pos"] + r["n_neg"] for r in level1 if r["group"] == 2) == 2 * 3          # three reads with sites, two letters
    # the descending order is exercised: read 1's mean differs in its last bits when summed the other way
    c, m = calls[1], maps[1]
    assert ref.read_mean(c["prob"][:, 0]) != ref.read_mean(c["prob"][::-1, 0]) or ref.read_mean(c["prob"][:, 1]) != ref.read_mean(c["prob"][::-1, 1])
    acc = sa.CallScores("CE", truth=lines, n_bins=N_BINS, threshold=THRESHOLD)
    acc.add_batch(b, maps)
    got_rows, got_curves, counts = _finish(acc)
    ref.check_rows(got_rows, got_curves, rows)
    assert counts["unlabelled"] == exp.unlabelled
    # the level-1 scores themselves, bit for bit: with one score per array the grid count is a step at the score
    acc.close()
    fine = sa.CallScores("CE", truth=lines, n_bins=1, threshold=0.0)
    only = [dict(m, true_letter=m["true_letter"] if j == 1 else -1) for j, m in enumerate(maps)]
    fine.add_batch(b, only)
    r1 = [r for r in fine.finish()[0] if r["level"] == 1 and r["group"] == 1]
    assert [(r["letter"], int(r["n_pos"]), int(r["n_neg"])) for r in r1] == [(b"C", 0, 1), (b"E", 1, 0)]
    fine.close()
    for l, letter in enumerate("CE"):                            # threshold = the expected mean: counted; its successor: not
        mean = ref.read_mean(c["prob"][::-1, l])                 # (mapped '-', x_sign +1: descending reference_index is descending x)
        for thr, n in ((mean, 1), (np.nextafter(mean, 2.0), 0)):
            t = sa.CallScores("CE", truth=lines, n_bins=1, threshold=float(thr))
            t.add_batch(b, only)
            r = [r for r in t.finish()[0] if r["level"] == 1 and r["group"] == 1 and r["letter"] == letter.encode()][0]
            assert int(r["tp"] + r["fp"]) == n, (letter, thr)
            t.close()


def _records(rng, n, decimals):
    p = rng.random(n)
    if decimals:
        p = np.round(p, decimals)
    return np.stack([p, 1.0 - p], axis=1), rng.integers(0, 2, n)


def test_records_cross_terms_additivity_and_rollback():
    rng = np.random.default_rng(3)
    exp = ref.Scores("CE", N_BINS, THRESHOLD)
    acc = sa.CallScores("CE", n_bins=N_BINS, threshold=THRESHOLD)
    two = sa.CallScores("CE", n_bins=N_BINS, threshold=THRESHOLD)
    for level, decimals in ((0, 0), (2, 6)):                     # level 2 as the CLI feeds it: six decimals, ties abound
        for strand in (0, 1):
            pa, ta = _records(rng, 3000 + 17 * strand, decimals)
            pb, tb = _records(rng, 900, decimals)
            pa[:4] = [[0.0, 1.0], [1.0, 0.0], [5e-324, 1.0], [-0.0, 1.0]]
            exp.add_records(level, strand, np.concatenate([pa, pb]), np.concatenate([ta, tb]))
            acc.add_records(level, strand, np.concatenate([pa, pb]), np.concatenate([ta, tb]))
            two.add_records(level, strand, pa, ta)               # add(A); add(B) is add(A + B)
            two.add_records(level, strand, pb, tb)
    rows = exp.rows()
    assert len(rows) == 12
    for level in (0, 2):                                         # the group of both strands is not the sum of its parts
        t, c, both = [[r for r in rows if r["level"] == level and r["group"] == g and r["letter"] == "C"][0] for g in range(3)]
        assert both["auc2"] > t["auc2"] + c["auc2"] and both["n_pos"] == t["n_pos"] + c["n_pos"]
    got = acc.finish()
    ref.check_rows(got[0], got[1], rows)
    assert got[2] == dict(unlabelled=0, other_sites=0)
    split = two.finish()
    assert split[0].tobytes() == got[0].tobytes() and split[1].tobytes() == got[1].tobytes()
    # checkpoint / rollback
    with pytest.raises(sa.SaError) as e:
        acc.rollback()
    assert e.value.code == -7                                    # SA_ESTATE: no checkpoint
    acc.checkpoint()
    acc.add_records(1, 0, *_records(rng, 500, 0))
    acc.add_records(0, 1, *_records(rng, 5000, 0))               # (grows an array past its room)
    assert acc.finish()[0].tobytes() != got[0].tobytes()
    acc.rollback()
    back = acc.finish()
    assert back[0].tobytes() == got[0].tobytes() and back[1].tobytes() == got[1].tobytes()
    acc.add_records(0, 1, *_records(rng, 10, 0))                 # usable after the rollback
    assert int(acc.finish()[0]["n_pos"].sum()) > int(got[0]["n_pos"].sum())
    acc.close()
    two.close()


def test_unlabelled_and_other_sites_counts():
    alpha, k, _, _ = synth.parse_model_table(cases.MODEL_CPG)
    pm = sa.Model.load(cases.MODEL_CPG)
    amb = {"X": "CE", "Y": "CT"}
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 3, 700, 200, cpg_ambiguous=True)
    for job in jobs:                                             # every third site gets other letters
        ref_l = list(job["ref"])
        for n, i in enumerate([i for i, ch in enumerate(ref_l) if ch == "X"]):
            if n % 3 == 1:
                ref_l[i] = "Y"
        job["ref"] = "".join(ref_l)
    b = sa.Batch(pm, sa.default_params(), jobs, ambig=sa.default_ambig(amb), flags=sa.FLAG_SITE_CALLS)
    b.run()
    calls = b.site_calls()
    maps = job_map(len(jobs))
    lines, table = positions_truth(jobs, maps, k, skip=3)
    exp = ref.Scores("CE", N_BINS, THRESHOLD)
    exp.add_site_calls(calls, maps, table)
    assert exp.other_sites > 5 and exp.unlabelled > 5 and exp.rows()
    acc = sa.CallScores("CE", truth=lines, n_bins=N_BINS, threshold=THRESHOLD)
    acc.add_batch(b, maps)
    acc.checkpoint()
    acc.add_batch(b, maps)                                       # the counts roll back with the arrays
    assert acc.finish()[2] == dict(unlabelled=2 * exp.unlabelled, other_sites=2 * exp.other_sites)
    acc.rollback()
    got = acc.finish()
    ref.check_rows(got[0], got[1], exp.rows())
    assert got[2] == dict(unlabelled=exp.unlabelled, other_sites=exp.other_sites)
    acc.close()
    no_truth = sa.CallScores("CE", n_bins=N_BINS, threshold=THRESHOLD)       # an empty table: every call is dropped
    no_truth.add_batch(b, maps)
    rows, _, counts = no_truth.finish()
    assert len(rows) == 0 and counts["unlabelled"] == sum(int((c["letters"] == "CE").sum()) for c in calls)
    no_truth.close()
    b.close()


def _code(fn, *a, **kw):
    with pytest.raises(sa.SaError) as e:
        fn(*a, **kw)
    return e.value.code


def test_error_contract():
    pm = sa.Model.load(cases.MODEL_CPG)
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 600, 120, cpg_ambiguous=True)
    amb = sa.default_ambig(CE)
    maps = job_map(2, labelled=(0, 1))
    acc = sa.CallScores("CE", truth=[(0, 5, 0, "C")], n_bins=N_BINS, threshold=THRESHOLD)
    b = sa.Batch(pm, p, jobs, ambig=amb)                          # without the flag
    b.run()
    assert _code(acc.add_batch, b, maps) == -7                   # SA_ESTATE
    b.close()
    b = sa.Batch(pm, p, jobs, ambig=amb, flags=sa.FLAG_SITE_CALLS)
    assert _code(acc.add_batch, b, maps) == -7                   # not run yet
    b.run()
    assert _code(acc.add_batch, b, maps[:1]) == -1               # SA_EINVAL: not the batch's number of jobs
    for field, bad in (("contig", -1), ("x_sign", 0), ("strand", 2), ("mapped_strand", -1), ("true_letter", 2), ("true_letter", -2)):
        assert _code(acc.add_batch, b, [maps[0], dict(maps[1], **{field: bad})]) == -1, field
    # records: a NaN, a value outside [0, 1], a level, a strand, a letter index
    good = np.array([[0.25, 0.75], [0.5, 0.5]])
    for prob, tl, level, strand in ((np.array([[0.25, np.nan]]), [0], 0, 0), (np.array([[0.25, 1.5]]), [0], 0, 0),
                                    (np.array([[-1e-9, 0.5]]), [0], 0, 0), (good, [0, 1], 3, 0), (good, [0, 1], 0, 2), (good, [0, 2], 0, 0),
                                    (good, [0, -1], 0, 0)):
        assert _code(acc.add_records, level, strand, prob, tl) == -1
    rows, _, counts = acc.finish()                               # a refused add adds nothing
    assert len(rows) == 0 and counts == dict(unlabelled=0, other_sites=0)
    acc.add_batch(b, maps)                                       # and the accumulator is still usable
    assert len(acc.finish()[0]) > 0
    acc.close()
    b.close()
    # create
    assert _code(sa.CallScores, "EC") == -1                      # not ascending
    assert _code(sa.CallScores, "C") == -1
    assert _code(sa.CallScores, "ABCDEFGHI") == -1
    assert _code(sa.CallScores, "CE", n_bins=0) == -1
    assert _code(sa.CallScores, "CE", threshold=float("nan")) == -1
    assert _code(sa.CallScores, "CE", truth=[(0, 5, 0, "T")]) == -1
    assert _code(sa.CallScores, "CE", truth=[(0, -5, 0, "C")]) == -1
    assert _code(sa.CallScores, "CE", truth=[(0, 5, 2, "C")]) == -1
    assert _code(sa.CallScores, "CE", device=99) == -1
