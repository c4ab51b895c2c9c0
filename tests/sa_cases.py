"""Shared test inputs: the same seeded jobs are handed to the CPU oracle and to the HIP library."""
import json
import os
import re

import numpy as np

from signalalign_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_6MER = os.path.join(GOLDEN, "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")
MODEL_CPG = os.path.join(GOLDEN, "models", "testModelR9.4_450bps.cpg.6mer.template.model")
MODEL_5MER = os.path.join(GOLDEN, "models", "testModelR9_5mer_acgt_template.model")
MODEL_R73 = os.path.join(GOLDEN, "models", "testModelR73_acegot_template.model")
NHDP = os.path.join(GOLDEN, "models", "templateSingleLevelFixed.nhdp")


def synthetic_jobs(model_path, n_reads, n_events, first_index=0, **kw):
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    return synth.make_jobs(n_reads, n_events, alpha, k, tab, first_index=first_index, **kw)


def realistic_anchor_jobs(model_path, n_reads, n_events, first_index=0, trim=14):
    """Synthetic reads whose anchors are thinned the way a real guide alignment thins them: match runs taken from
    the bundled minus-strand cigar (tests/golden/cigars), `trim` anchors dropped at both ends of each run, nothing
    kept inside deletions.  About one base in six stays an anchor and most diagonals are wider than 64 lanes."""
    return thin_anchors_like_a_guide_alignment(synthetic_jobs(model_path, n_reads, n_events, first_index), trim)


def thin_anchors_like_a_guide_alignment(job_list, trim=14):
    """the thinning of realistic_anchor_jobs for any list of jobs (HDP reads too)"""
    toks = open(os.path.join(GOLDEN, "cigars", "ecoli_minus_strand.cigar")).read().split()[10:]
    runs = [(toks[i], int(toks[i + 1])) for i in range(0, len(toks), 2)]
    jobs = []
    for j, job in enumerate(job_list):
        ax, ay = job["ax"], job["ay"]
        keep = np.zeros(len(ax), dtype=bool)
        pos, r = 0, (7 * j) % len(runs)
        while pos < len(ax):
            op, ln = runs[r % len(runs)]
            r += 1
            if op == "M":
                if ln > 2 * trim:
                    keep[pos + trim: min(pos + ln - trim, len(ax))] = True
                pos += ln
            elif op == "D":
                pos += ln
        q = dict(job)
        q["ax"], q["ay"] = ax[keep], ay[keep]
        jobs.append(q)
    return jobs


def oracle_pairs(oracle, omodel, job, params, ambig=None):
    omodel.set_read_params(job["scale"], job["shift"], job["var"])
    return oracle.align(omodel, job["ref"], job["events"], job["ax"], job["ay"], params, ambig=ambig, ragged=job.get("ragged", (1, 1)))


def oracle_params(oracle, p):
    """translate a signalalign_amd.Params into the oracle's Params"""
    return oracle.Params(p.threshold, p.diagonal_expansion, p.trace_back_diagonals, p.min_diags_between_trace_back,
                         p.split_matrix_bigger_than_this, 14)


def check_plan_geometry(oracle, sa, model, k, p, job, tag=None, ambig=None, flags=0):
    """The host planner's view of one job (sa.plan_describe) against the oracle: its regions are getSplitPoints' and every band row of
    every region is band_construct's for the anchors of that region.  Returns what plan_describe returned."""
    ax, ay = np.asarray(job["ax"], dtype=np.int64), np.asarray(job["ay"], dtype=np.int64)
    lX, lY = len(job["ref"]) - (k - 1), len(job["events"])
    rl, rr = job.get("ragged", (1, 1))
    info, regions, rows, segs = sa.plan_describe(model, p, job, ambig=ambig, flags=flags)
    exp_regions = oracle.split_points(ax, ay, lX, lY, p.split_matrix_bigger_than_this, rl, rr)
    assert np.array_equal(regions, exp_regions), tag
    off = 0
    for r, (x1, y1, x2, y2) in enumerate(regions):
        sel = (ax + ay >= x1 + y1) & (ax + ay < x2 + y2)
        L, R = oracle.band(ax[sel] - x1, ay[sel] - y1, x2 - x1, y2 - y1, p.diagonal_expansion)
        n = len(L)
        assert np.array_equal(rows[off:off + n, 1], L) and np.array_equal(rows[off:off + n, 2], R), (tag, r)
        off += n
    return info, regions, rows, segs


def npread_job(oracle, npread_name, model_path, reference=None):
    """A bundled .npRead aligned to `reference` (default: its own template read) with a single-M guide
    alignment: the substitution for BASELINE config 1 described in SURVEY.md section 8(c)."""
    r = oracle.parse_npread(os.path.join(GOLDEN, "npReads", npread_name))
    om = oracle.Model.from_file(model_path)
    ev = r["template_events"].copy()
    read = r["template_read"]
    pr = oracle.estimate_params(om, r["template_strand_event_map"], ev, read)
    ref = reference if reference is not None else read
    L = min(len(ref), len(read))
    gx, gy = oracle.guide_to_anchors(0, L, 1, 0, [(0, L)], 14)
    em = r["template_strand_event_map"]
    ax, ay = oracle.remap_anchors(gx, gy, em, 0)
    lo, hi = int(em[0]), int(em[L - 1])
    return dict(ref=ref[:L], events=np.ascontiguousarray(ev[lo:hi]), ax=ax, ay=ay, scale=pr["scale"],
                shift=pr["shift"], var=pr["var"])


def compare_pairs(got, exp, tol_e7, threshold):
    """got/exp: structured arrays.  Rows must agree on (x, y, path) and differ by at most tol_e7 in prob_e7,
    except rows whose probability is within tol of the threshold (they may appear on one side only).
    Returns (max_abs_diff_e7, n_only_one_side)."""
    def key(a):
        return {(int(r["x"]), int(r["y"]), int(r["path"])): int(r["prob_e7"]) for r in a}
    g, e = key(got), key(exp)
    assert len(g) == len(got) and len(e) == len(exp), "duplicate (x,y,path) rows"
    worst, lonely = 0, 0
    thr_e7 = threshold * 1e7
    for k, v in e.items():
        if k in g:
            worst = max(worst, abs(g[k] - v))
        else:
            assert abs(v - thr_e7) <= tol_e7 + 1, ("missing pair", k, v)
            lonely += 1
    for k, v in g.items():
        if k not in e:
            assert abs(v - thr_e7) <= tol_e7 + 1, ("extra pair", k, v)
            lonely += 1
    assert worst <= tol_e7, ("posterior differs by more than the tolerance", worst)
    return worst, lonely


def same_order(got, exp):
    """rows present on both sides appear in the same relative order"""
    ke = [(int(r["x"]), int(r["y"]), int(r["path"])) for r in exp]
    kg = [(int(r["x"]), int(r["y"]), int(r["path"])) for r in got]
    se, sg = set(ke), set(kg)
    return [k for k in ke if k in sg] == [k for k in kg if k in se]


_HDP_CACHE = {}


def hdp_jobs(n_reads, n_events, first_index=0, table5=None):
    """Reads of the HDP workload (BASELINE configs[3]): reference assembled from windows of the sequence the bundled .nhdp was
    trained on, events drawn from the density the aligner itself uses for each k-mer (synth.make_read_hdp).  table5: the
    model's table after set_to_hdp_expected_values (sa.Model.table5() or the oracle's match_table())."""
    if "sampler" not in _HDP_CACHE:
        _HDP_CACHE["sampler"] = synth.HdpSampler(synth.parse_nhdp(NHDP))
        _HDP_CACHE["pool"] = open(os.path.join(GOLDEN, "npReads", "ZymoRef.txt")).read().split()[0].strip()
    alpha, k, t10, tab = synth.parse_model_table(MODEL_R73)
    t5 = tab if table5 is None else np.asarray(table5)
    return [synth.make_read_hdp(first_index + i, n_events, alpha, k, t5, _HDP_CACHE["sampler"], _HDP_CACHE["pool"])
            for i in range(n_reads)]


def events_for_sequence(seq, model_path, seed):
    """Synthetic events for a given nucleotide sequence (as synth.make_read draws them for a random one): 0-7 events per
    k-mer, means ~ N(mu_k, sd_k).  Returns (events4, event_map) with event_map[i] = first event of the k-mer at base i."""
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    alpha = "".join(sorted(alpha))
    rng = np.random.Generator(np.random.PCG64(seed))
    n_kmers = len(seq) - k + 1
    digit = np.array([alpha.index(c) for c in seq], dtype=np.int64)
    kid = np.zeros(n_kmers, dtype=np.int64)
    for i in range(k):
        kid = kid * len(alpha) + digit[i:i + n_kmers]
    p = synth.EVENTS_PER_KMER_P / synth.EVENTS_PER_KMER_P.sum()
    counts = rng.choice(len(p), size=n_kmers, p=p)
    counts[0] = max(counts[0], 1)
    owner = np.repeat(np.arange(n_kmers), counts)
    E = len(owner)
    means = rng.normal(tab[5 * kid[owner]], tab[5 * kid[owner] + 1])
    noise = np.abs(rng.normal(tab[5 * kid[owner] + 2], tab[5 * kid[owner] + 3])) + 1e-3
    dur = np.full(E, 0.00127)
    events4 = np.ascontiguousarray(np.stack([means, noise, dur, np.cumsum(dur) - dur], axis=1))
    first = np.cumsum(counts) - counts
    idx = np.maximum.accumulate(np.where(counts > 0, np.arange(n_kmers), 0))
    emap = np.full(len(seq), E - 1, dtype=np.int64)
    emap[:n_kmers] = np.minimum(first[idx], E - 1)
    return events4, emap


def write_npread_1d(path, read, event_map, events4):
    """A 1-D .npRead as nanopore_loadNanoporeReadFromFile reads it (impl/nanopore.c:145-521; layout of the bundled
    tests/test_npReads/r9p4_oneD.npRead): header, empty 2-D read, template read, template strand event map, three empty
    complement lines, the template events, empty lines."""
    with open(path, "w") as f:
        f.write("0 %d 0 %d 0 1 1 1 1 1 0 1 1 1 1 1 0 0\n" % (len(events4), len(read)))
        f.write("\n%s\n%s\n\n\n\n" % (read, " ".join(str(int(v)) for v in event_map)))
        f.write(" ".join(repr(float(v)) for v in np.asarray(events4).reshape(-1)) + "\n")
        f.write("\n\n\n\n\n\n\n")


# What the reference ran with when it wrote the posteriors of its bundled reads (tests/golden/expected/reference_output_*.npz):
# threshold, diagonal expansion, traceBackDiagonals, minDiagsBetweenTraceBack, splitMatrixBiggerThanThis, constraint trim.  The
# traceback length is pairwiseAlignmentBandingParameters_construct's 40 (impl/pairwiseAligner.c:2026), not the 50 signalMachine's
# -g defaults to nor the 100 the Python driver passes: only 40 reproduces the rows of the E. coli 1-D read (39 and 41 do not).
REFERENCE_RUN = dict(threshold=0.01, expansion=50, trace_back=40, min_diags=1000, split=3000 * 3000, trim=14)
ECOLI1D_MODEL = os.path.join(GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")


def reference_run_params(oracle, trace_back=None):
    """REFERENCE_RUN as the oracle's Params (trace_back: another traceback length, for the controls)"""
    q = REFERENCE_RUN
    return oracle.Params(q["threshold"], q["expansion"], q["trace_back"] if trace_back is None else trace_back, q["min_diags"],
                         q["split"], q["trim"])


def sam_cigar_operations(cigar):
    """A SAM CIGAR as (read start, [(operation, length)]): leading S = the read's first aligned base, M/D/I = operations 0/1/2 of
    sa_guide_to_anchors (D consumes reference, I consumes read), a trailing S is dropped."""
    toks = re.findall(r"([0-9]+)([A-Z=])", cigar)
    assert "".join(n + c for n, c in toks) == cigar and all(c in "SMDI" for _, c in toks), cigar
    start = int(toks[0][0]) if toks[0][1] == "S" else 0
    body = toks[1 if toks[0][1] == "S" else 0: len(toks) - (toks[-1][1] == "S")]
    assert all(c != "S" for _, c in body)
    return start, [({"M": 0, "D": 1, "I": 2}[c], int(n)) for n, c in body]


def reference_output_ecoli1d_inputs(oracle, unknown="A"):
    """The reference's output for the bundled R9.4 1-D read (tests/golden/expected/reference_output_ecoli1d.npz) as an alignment
    job: (posteriors by (window position, event), reference window rebuilt from the rows' k-mers, parsed .npRead, (start1, end1,
    start2, end2), guide-alignment operations).  The E. coli genome is a missing blob, so the window comes from the rows; the guide
    alignment is the one the file was made with, bwa's (tests/golden/cigars/r9p4_oneD_bwa.json: 42S30M1D11M...2S at POS 3560629,
    i.e. read 42-6540 on window 0-6817).  With it, REFERENCE_RUN and the two-distribution emission the CPU restatement gives the
    file's 11,892 cells and no other, every posterior within the print precision (tests/test_oracle_reference_outputs.py).
    unknown: the letter for the one window base no row covers (index 6138); only A reproduces the file."""
    z = np.load(os.path.join(GOLDEN, "expected", "reference_output_ecoli1d.npz"))
    gold = {(int(x), int(y)): float(p) for x, y, p in zip(z["x"], z["y"], z["p"])}
    assert str(z["window"]).count("?") == 1
    window = str(z["window"]).replace("?", unknown)
    r = oracle.parse_npread(os.path.join(GOLDEN, "npReads", "r9p4_oneD.npRead"))
    bwa = json.load(open(os.path.join(GOLDEN, "cigars", "r9p4_oneD_bwa.json")))
    assert bwa["flag"] == 0
    s2, ops = sam_cigar_operations(bwa["cigar"])
    s1 = bwa["pos"] - 1 - int(z["first_position"])
    e1 = s1 + sum(n for t, n in ops if t != 2)
    e2 = s2 + sum(n for t, n in ops if t != 1)
    assert (s1, e1, s2, e2) == (0, len(window), 42, 6540) and e1 == 6817
    return gold, window, r, (s1, e1, s2, e2), ops


def against_reference_rows(mine, gold):
    """A run's {(x, y): p} against the reference's: (rows of the reference that are missing, rows the reference has not, worst
    |dp| over the common rows)."""
    missing = sorted(set(gold) - set(mine))
    extra = sorted(set(mine) - set(gold))
    worst = max([abs(mine[k] - gold[k]) for k in set(mine) & set(gold)] + [0.0])
    return missing, extra, worst


# the reference prints six decimals (half a unit: 5e-7); prob_e7 carries the posterior in units of 1e-7
PRINT_PRECISION = 5e-7 + 1e-7


def check_reference_rows(mine, gold, kernel_error, tag):
    """The bars of a run against the rows the reference printed.  kernel_error 0 (the restatement, the reference-ordered kernels):
    the reference's set exactly, every posterior within the print precision.  kernel_error 1e-5 (the register kernels' contract):
    every row of the reference present -- none of its posteriors is within 1e-5 of the threshold -- at most two rows it has not,
    each below threshold + 1e-5 (the reference has three cells within 2.4e-5 under the threshold, two of them within 1e-5), and
    every posterior within 1e-5 plus the print precision.  Prints and returns (missing, extra, worst |dp|)."""
    missing, extra, worst = against_reference_rows(mine, gold)
    print("%s against the reference's rows: %d rows, %d missing, %d extra, max |dp| %.3g" % (tag, len(mine), len(missing), len(extra), worst))
    assert not missing, (tag, len(missing), missing[:5])
    if kernel_error == 0:
        assert not extra, (tag, len(extra), extra[:5])
    else:
        assert len(extra) <= 2 and all(mine[k] < REFERENCE_RUN["threshold"] + kernel_error for k in extra), (tag, [(k, mine[k]) for k in extra[:5]])
    assert worst <= kernel_error + PRINT_PRECISION, (tag, worst)
    return missing, extra, worst


def reference_residual(mine, gold):
    """How a run's posteriors compare with the ones the reference printed (round 4, probes/reference_output_residuals.py).
    The rows that differ by more than 1e-4 do not sit at band edges: they come in groups of consecutive diagonals that share ONE
    multiplicative factor, |log factor| <= 1.5e-3 -- the total probability a posterior is divided by.  The reference refreshes
    that total on every tenth diagonal of a traceback, and its approximate logAdd makes the total depend on the diagonal it is
    evaluated on (un-banded restatement on the Zymo read: totals ten diagonals apart differ by 6e-5 in the median, 5e-4 at the
    95th percentile, 1.7e-3 at most); which diagonals those are depends on where the tracebacks fire, i.e. on the guide
    alignment, which for the Zymo read is lastz's and not the one the file was made with.  So the bar that the explanation supports is RELATIVE:
    |dp| <= 1.5e-3 p + 2e-6 (the print precision).  Returns (share of the reference's rows found, median |dp|, share of the found
    rows within that bar, share within 1e-4 absolute, the rows beyond the bar as (x + y, x, y, reference p, this run's p))."""
    common = sorted(set(mine) & set(gold))
    g = np.array([gold[k] for k in common])
    m = np.array([mine[k] for k in common])
    d = np.abs(m - g)
    ok = d <= 1.5e-3 * np.maximum(g, m) + 2e-6
    beyond = [(k[-2] + k[-1], k[-2], k[-1], float(gg), float(mm)) for k, gg, mm, o in zip(common, g, m, ok) if not o]
    return len(common) / max(len(gold), 1), float(np.median(d)), float(ok.mean()), float((d <= 1e-4).mean()), beyond
