"""sa_guide_align_batch on the GPU against tests/guide_ref.py's band-by-band restatement: status, score, the four ends and the
operations are compared bit for bit.  The restatement's answers are computed once per (read, window, diag, band) and shared
(guide_ref.banded_cached)."""
import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import guide_ref as g
import sa_cases as cases

pytestmark = pytest.mark.gpu

FIELDS = ("status", "score", "read_start", "read_end", "ref_start", "ref_end", "ops")


def rand_seq(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(4, size=n))


def check(jobs, band=128):
    """one batch on the device, every job against the restatement; returns the device's results"""
    jobs = [(j[0], j[1], j[2] if len(j) > 2 else 0) for j in jobs]
    got = sa.guide_align_batch(jobs, sa.guide_params(band=band))
    assert len(got) == len(jobs)
    for k, (job, res) in enumerate(zip(jobs, got)):
        exp = g.banded_cached(job[0], job[1], job[2], band)
        for f in FIELDS:
            assert res[f] == exp[f], (k, f, len(job[0]), len(job[1]), job[2], band, res[f] if f != "ops" else res[f][:8],
                                      exp[f] if f != "ops" else exp[f][:8])
    return got


@pytest.mark.parametrize("band", [64, 128, 256])
def test_the_two_real_pairs(band):
    got = check([g.ecoli_pair(), g.zymo_pair()], band)
    assert got[0]["status"] == 0 and got[0]["read_start"] == 42      # bwa soft-clipped 42 bases as well
    assert got[1]["status"] == 0


EDGE = (1, 2, 63, 64, 65, 127, 128, 129, 191, 193)


def edge_jobs(other):
    """read or window length on the refill of a 64-entry buffer and on the hand-over lanes, the other sequence `other` long:
    the short one is a mutated piece of the long one"""
    rng = np.random.Generator(np.random.PCG64(77 + other))
    jobs = []
    for L in EDGE:
        long_seq = rand_seq(rng, other)
        a = int(rng.integers(0, max(other - L, 0) + 1))
        piece = g.mutate(rng, long_seq[a:a + L + 8], rate=0.08)[:L]
        piece = piece + rand_seq(rng, L - len(piece))
        jobs.append((piece, long_seq, a))          # short read, long window, placed
        jobs.append((long_seq, piece, 0))          # long read, short window
    return jobs


@pytest.mark.parametrize("band", [64, 128, 192, 256])
def test_lengths_on_the_buffer_and_lane_boundaries_against_100(band):
    check(edge_jobs(100), band)


def test_lengths_on_the_buffer_and_lane_boundaries_against_1000():
    check(edge_jobs(1000), 128)


def test_shapes_where_the_kernel_can_go_wrong():
    rng = np.random.Generator(np.random.PCG64(5))
    ref = rand_seq(rng, 900)
    read = g.mutate(rng, ref, rate=0.1)
    jobs, name = [], {}

    def add(label, *job):
        name[label] = len(jobs)
        jobs.append(job)
    add("window shorter than the band", g.mutate(rng, ref[100:400], rate=0.05), ref[230:270])
    add("diag > 0", read, rand_seq(rng, 500) + ref, 500)
    add("band 0 partly left of the matrix", read, ref, 10)
    add("band 0 partly right of the matrix", read[:60], ref, len(ref) - 5)
    add("diag beyond the window is clamped", read[:60], ref, len(ref) + 1000)
    add("negative diag is clamped", read, ref, -7)
    add("identical", ref, ref)
    add("no positive score", "A" * 200, "C" * 150)
    add("empty read", "", ref)
    add("empty window", read, "")
    add("deletion of 40", ref[:400] + ref[440:], ref)
    add("insertion of 40", ref[:400] + rand_seq(rng, 40) + ref[400:], ref)
    lower = read.lower()
    add("lower case", lower, ref)
    spiced = list(ref)
    for k in range(30, len(spiced), 41):
        spiced[k] = "N" if k % 2 else "E"
    add("N and E letters", read, "".join(spiced))
    add("n in the read", read[:300] + "n" + read[301:], ref)
    add("ends mid-read", g.mutate(rng, ref[:300], rate=0.05) + rand_seq(rng, 200), ref)
    got = check(jobs, 128)
    r = lambda label: got[name[label]]
    assert r("identical")["ops"] == [(0, len(ref))] and r("identical")["score"] == 2 * len(ref) and r("identical")["status"] == 0
    assert r("no positive score")["status"] & sa.GUIDE_NO_ALIGNMENT and r("no positive score")["ops"] == []
    assert r("empty read")["status"] == sa.GUIDE_EMPTY and r("empty window")["status"] == sa.GUIDE_EMPTY
    assert (1, 40) in r("deletion of 40")["ops"] and r("deletion of 40")["score"] == 2 * 860 - (4 + 2 * 40)
    assert (2, 40) in r("insertion of 40")["ops"] and r("insertion of 40")["score"] == 2 * 900 - (4 + 2 * 40)
    assert r("lower case")["score"] == g.banded_cached(read, ref, 0, 128)["score"]
    assert r("ends mid-read")["read_end"] < 400 and r("ends mid-read")["status"] == 0
    assert r("diag > 0")["ref_start"] >= 480
    assert r("window shorter than the band")["status"] & sa.GUIDE_SHORT


def mixed_jobs():
    rng = np.random.Generator(np.random.PCG64(33))
    jobs = []
    for k in range(33):
        L = int(rng.integers(30, 700))
        ref = rand_seq(rng, L)
        kind = k % 4
        if kind == 0:
            jobs.append((g.mutate(rng, ref, rate=0.1), ref, 0))
        elif kind == 1:
            pad = int(rng.integers(1, 300))
            jobs.append((g.mutate(rng, ref, rate=0.05), rand_seq(rng, pad) + ref + rand_seq(rng, 40), pad))
        elif kind == 2:
            jobs.append((rand_seq(rng, int(rng.integers(1, 90))), ref, int(rng.integers(0, L))))
        else:
            jobs.append((g.mutate(rng, ref, rate=0.15)[: L // 2], ref, 0))
    jobs[7] = ("", jobs[7][1], 0)
    return jobs


def test_a_batch_equals_its_jobs_one_at_a_time_and_scratch_is_reused(monkeypatch):
    jobs = mixed_jobs()
    prm = sa.guide_params()
    sa.guide_release()
    small = sa.guide_align_batch(jobs[:3], prm)            # a small call first: the next one grows the scratch
    first = sa.guide_align_batch(jobs, prm)
    second = sa.guide_align_batch(jobs, prm)               # ... and this one reuses it
    assert first == second and first[:3] == small
    single = [sa.guide_align_batch([j], prm)[0] for j in jobs]
    assert single == first
    sa.guide_release()
    assert sa.guide_align_batch(jobs, prm) == first
    monkeypatch.setenv("SA_GUIDE_TRACE_MB", "0.05")        # several slices
    assert sa.guide_align_batch(jobs, prm) == first
    monkeypatch.delenv("SA_GUIDE_TRACE_MB")
    check(jobs, 128)


def test_the_synthetic_pairs_in_one_batch():
    got = check(list(g.synthetic_pairs()), 128)
    assert all(r["status"] == 0 for r in got)


def test_argument_checks_come_before_the_device():
    with pytest.raises(sa.SaError):
        sa.guide_align_batch([("ACGT", "ACGT")], sa.guide_params(band=100))
    with pytest.raises(sa.SaError):
        sa.guide_align_batch([("ACGT", "ACGT")], sa.guide_params(gap_extend=0))


# What the GPU's own guide alignment reaches on this read at the reference's traceBackDiagonals 40, measured on the MI355X (DESIGN.md,
# "Guide alignment"): the share of the reference's rows found, of the found rows within 1e-4 and within the relative bar of
# sa_cases.reference_residual.  The bars are 0.01 below, and never under the CPU bars of
# tests/test_oracle_reference_outputs.py::test_r9p4_one_d_posteriors_with_the_restated_guide_alignment, which runs the same job
# on the restatement's (bit-identical) alignment.
E2E_FOUND, E2E_WITHIN_1E4, E2E_WITHIN_REL = 0.9993, 0.9961, 0.9995
CPU_FOUND, CPU_WITHIN_1E4, CPU_WITHIN_REL, CPU_EXTRA = 0.989, 0.986, 0.989, 0.002


def test_the_gpu_guide_alignment_carries_the_ecoli_read_to_the_reference_posteriors(oracle):
    """End to end: sa_guide_align_batch's alignment of the bundled R9.4 1-D read -> sa_guide_to_anchors -> the register kernels,
    run as the reference ran (sa_cases.REFERENCE_RUN) and compared with the posteriors it printed.
    tests/test_gpu_reference_outputs.py does the same with bwa's alignment, which reproduces the file whole."""
    gold, window, r, _, _ = cases.reference_output_ecoli1d_inputs(oracle)
    read = r["template_read"]
    res = sa.guide_align_batch([(read, window)])[0]
    assert res["status"] == 0
    s1, e1, s2, e2, ops = res["ref_start"], res["ref_end"], res["read_start"], res["read_end"], res["ops"]
    alpha, k, t10, tab = synth.parse_model_table(cases.ECOLI1D_MODEL)
    em = r["template_strand_event_map"]
    pm0 = sa.Model.load(cases.ECOLI1D_MODEL)
    ev = r["template_events"].copy()
    t5 = np.array(pm0.table5()).copy()
    pr = sa.estimate_params(pm0, t5, em, ev, read)
    q = cases.REFERENCE_RUN
    gx, gy = sa.guide_to_anchors(s1, e1, 1, s2, ops, q["trim"])
    ax, ay = sa.remap_anchors(gx, gy, em, s2)
    lo, hi = int(em[s2]), int(em[e2 - 1])
    pm = sa.Model.create(alpha, k, t10, t5)
    pm.set_emission(1)
    p = sa.default_params(threshold=q["threshold"], expansion=q["expansion"], trace_back=q["trace_back"])
    job = dict(ref=window[s1:e1], events=np.ascontiguousarray(ev[lo:hi]), ax=ax, ay=ay, scale=pr["scale"], shift=pr["shift"], var=pr["var"])
    bf = sa.Batch(pm, p, [job])
    bf.run()
    got = bf.pairs(0)
    assert bf.stats().n_fast_regions == bf.stats().n_regions >= 1
    bf.close()
    mine = {(int(q_["x"]) + s1, int(q_["y"]) + lo): int(q_["prob_e7"]) / 1e7 for q_ in got}
    found, median, within_rel, within_1e4, _ = cases.reference_residual(mine, gold)
    extra = len(set(mine) - set(gold))
    print("guide e2e at trace_back %d: found %.4f extra rows %d median %.3g within_rel %.4f within_1e-4 %.4f"
          % (q["trace_back"], found, extra, median, within_rel, within_1e4))
    assert found >= max(CPU_FOUND, E2E_FOUND - 0.01) and within_1e4 >= max(CPU_WITHIN_1E4, E2E_WITHIN_1E4 - 0.01)
    assert median <= 5e-6 and within_rel >= max(CPU_WITHIN_REL, E2E_WITHIN_REL - 0.01) and extra <= CPU_EXTRA * len(gold)
