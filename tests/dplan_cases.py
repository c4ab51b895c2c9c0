"""Inputs at the edges of the device planner's own walk (signalalign_amd/csrc/sa_dplan.inc): data only.

The device planner walks a read with 256-thread strided loops, workgroup scans that carry a sum from one 256-wide step to the
next, a binary search over the anchors' x + y (in LDS up to 8192 anchors, in global memory beyond) and a 1024-read tile loop
over the batch.  CASES puts reads and batches on those boundaries.  tests/test_host_dplan_cases.py pins each case to the CPU
oracle through the host planner (no GPU), tests/test_gpu_dplan_edges.py compares the device planner's bytes with the host
planner's.  With lX = len(ref) - (k - 1), lY = number of events, N = lX + lY: a read has diagonals 0 .. N.

Every case carries the answer sa.dplan_compare must give, written out in the table: 0 (taken by the device planner and
identical to the host planner's arrays) or NOT_TAKEN.  Jobs are built once per process and shared: do not modify them."""
import functools
from collections import namedtuple

import numpy as np

from signalalign_amd import synth

import sa_cases as cases

NOT_TAKEN = 1 << 30
FLAG_EXPECT_INTERNAL = 0x10000

# model key -> (.model file, .nhdp file or None)
MODELS = {"6mer": (cases.MODEL_6MER, None), "5mer": (cases.MODEL_5MER, None), "cpg": (cases.MODEL_CPG, None),
          "r73hdp": (cases.MODEL_R73, cases.NHDP)}

# name; group of the list in DESIGN.md ("Planner on the device"); model key; keyword arguments of sa.default_params; the builder of
# the jobs as (function, arguments); ambiguity table (None: the default one); flags; environment; the answer of sa.dplan_compare
Case = namedtuple("Case", "name group model params build ambig flags env expect")


@functools.lru_cache(maxsize=None)
def _table(model):
    return synth.parse_model_table(MODELS[model][0])


def kmer_length(model):
    return _table(model)[1]


def _cut(r, k, lX, lY):
    """the first lX k-mers and lY events of a synth.make_read read, with the anchors that stay inside the matrix"""
    assert len(r["ref"]) - (k - 1) >= lX and len(r["events"]) >= lY, (len(r["ref"]), len(r["events"]), lX, lY)
    keep = (r["ax"] < lX) & (r["ay"] < lY)
    return dict(ref=r["ref"][:lX + k - 1], events=np.ascontiguousarray(r["events"][:lY]), ax=r["ax"][keep].copy(),
                ay=r["ay"][keep].copy(), scale=r["scale"], shift=r["shift"], var=r["var"])


def shaped_read(model, index, lX, lY, trim=14):
    """a read of exactly lX k-mers and lY events, dense anchors (every base from `trim` on, as far as both fit)"""
    alpha, k, t10, tab = _table(model)
    r = synth.make_read(index, int(max(lY, 1.67 * lX) * 1.15) + 60, alpha, k, tab, trim=trim)
    return _cut(r, k, lX, lY)


def read_of_events(model, index, n_events, trim=14):
    """a read of exactly n_events events and the k-mers that emitted them, dense anchors"""
    alpha, k, t10, tab = _table(model)
    r = synth.make_read(index, n_events + 40, alpha, k, tab, trim=trim)
    n_kmers = len(r["ref"]) - (k - 1)
    lX = int(np.searchsorted(r["event_map"][:n_kmers], n_events, side="left"))
    return _cut(r, k, max(lX, 1), n_events)


def _with_anchors(job, pairs):
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return dict(job, ax=np.ascontiguousarray(a[:, 0]), ay=np.ascontiguousarray(a[:, 1]))


def dims(job, k):
    return len(job["ref"]) - (k - 1), len(job["events"])


# ---- group 1: the number of diagonals on the 256-thread stride ---------------------------------------------------------------
G1_DIAGONALS = (255, 256, 257, 511, 512, 513, 769)     # N + 1
G1_LX = (255, 256, 257)                                # at lY = 300


@functools.lru_cache(maxsize=None)
def g1_jobs(model):
    jobs = []
    for i, nd in enumerate(G1_DIAGONALS):
        N = nd - 1
        lX = int(round(N / 2.67))
        jobs.append(shaped_read(model, 1000 + i, lX, N - lX))
    for i, lX in enumerate(G1_LX):
        jobs.append(shaped_read(model, 1100 + i, lX, 300))
    return jobs


# ---- group 2: path tables on the stride (CpG model, X -> C / E) ----------------------------------------------------------------
# The path-offset scan takes cells x = 1 .. 256, 257 .. 512, 513 ..: what must carry is poff[257] and poff[513].  A window (cell x
# holds ref[x - 1 .. x + 4]) with one X has 2 paths, with two 4.  X at 256 and 258: cells 254 .. 257 have 4 paths; X at 256 alone:
# cells 252 .. 257 have 2; no X near: 1 path on both sides of the step.
G2_LX = (255, 256, 257, 513)
G2_PLACEMENTS = ((256, 258), (256,), (100,))
G2_AMBIG = {"X": "CE"}


def _put_x(job, positions):
    ref = list(job["ref"])
    for p in positions:
        ref[p] = "X"
    return dict(job, ref="".join(ref))


@functools.lru_cache(maxsize=None)
def g2_jobs():
    jobs, idx = [], 2000
    for lX in G2_LX:
        for pl in G2_PLACEMENTS:
            base = shaped_read("cpg", idx, lX, int(lX * 1.6))
            idx += 1
            pos = [p for p in pl if p < len(base["ref"])]
            if lX > 512:   # the same around the second step, one placement further on: 2 paths at 256 | 257 come with 4 at 512 | 513
                nxt = G2_PLACEMENTS[(G2_PLACEMENTS.index(pl) + 2) % 3]
                pos += [p + 256 for p in nxt if p + 256 < len(base["ref"])]
            jobs.append(_put_x(base, pos))
    first = shaped_read("cpg", idx, 256, 400)
    jobs.append(_put_x(first, [0]))                          # the only X is the first letter of the reference
    last = shaped_read("cpg", idx + 1, 257, 400)
    jobs.append(_put_x(last, [len(last["ref"]) - 1]))        # ... the last letter
    return jobs


# ---- group 3: anchor lists -----------------------------------------------------------------------------------------------------
G3_BIG = (8191, 8192, 8193)        # anchors: ax = ay = arange(n), lX = lY = n + 7; 8192 is what the LDS search holds
G3_RUN, G3_STRETCH = 100, 300      # a run of (x + 1, y + 1) anchors, then nothing: the band stays under 512 cells


@functools.lru_cache(maxsize=None)
def g3_lists(model):
    base = shaped_read(model, 3000, 120, 200)
    a = np.stack([base["ax"], base["ay"]], axis=1)
    assert len(a) >= 40
    jobs = [_with_anchors(base, []),                                                     # 0 anchors
            _with_anchors(base, [a[len(a) // 2]]),                                       # 1
            _with_anchors(base, [a[10], a[-10]]),                                        # 2
            _with_anchors(base, [(0, 0)] + [tuple(q) for q in a if q[0] > 0 and q[1] > 0]),            # the first one at (0, 0)
            _with_anchors(base, [tuple(q) for q in a if q[0] < 119 and q[1] < 199] + [(119, 199)])]    # the last at (lX - 1, lY - 1)
    run = shaped_read(model, 3001, G3_RUN + G3_STRETCH, G3_RUN + G3_STRETCH)
    jobs.append(_with_anchors(run, [(i, i) for i in range(G3_RUN)]))
    return jobs


@functools.lru_cache(maxsize=None)
def _g3_big_read(n):
    return _with_anchors(shaped_read("6mer", 3100 + n, n + 7, n + 7), np.stack([np.arange(n), np.arange(n)], axis=1))


def g3_big(*counts):
    return [_g3_big_read(n) for n in counts]


@functools.lru_cache(maxsize=None)
def g3_big_own_anchors():
    """8193 anchors again, the read's own this time (y rises by 0 to 7 events per base).  On anchors that lie on one straight line
    the band is the same stripe whichever anchor a diagonal's search returns; here a search that is one anchor off gives another row."""
    alpha, k, t10, tab = _table("6mer")
    r = synth.make_read(3099, 15500, alpha, k, tab)
    n = G3_BIG[-1]
    assert len(r["ax"]) > n
    job = _cut(r, k, int(r["ax"][n - 1]) + 8, int(r["ay"][n - 1]) + 8)
    return [dict(job, ax=job["ax"][:n].copy(), ay=job["ay"][:n].copy())]


# ---- group 4: the traceback schedule -------------------------------------------------------------------------------------------
G4_EVENTS = (400, 1000, 1001, 1100, 4000)
G4_MIN_DIAGS = 300                                     # reads with N = min_diags - 1 .. min_diags + 2


@functools.lru_cache(maxsize=None)
def g4_reads(model, *n_events):
    return [read_of_events(model, 4000 + n, n) for n in n_events]


@functools.lru_cache(maxsize=None)
def g4_on_min_diags(model):
    jobs = []
    for i, N in enumerate(range(G4_MIN_DIAGS - 1, G4_MIN_DIAGS + 3)):
        lX = 112
        jobs.append(shaped_read(model, 4100 + i, lX, N - lX))
    return jobs


# ---- group 5: the batch on the 256-read scan step and the 1024-read tile ----------------------------------------------------------
G5_SIZES = (255, 256, 257, 1023, 1024, 1025, 2049)
# forward-storage budget (SA_F_BUDGET_CELLPATHS) for the 2049-read batch: tests/test_host_dplan_cases.py asserts from the host
# plan that it gives at least 40 passes and that a pass ends between reads 1023 and 1025
G5_BUDGET = 125000


@functools.lru_cache(maxsize=None)
def _g5_pool():
    rng = np.random.default_rng(5)
    tiny, wide = [], []
    for i in range(max(G5_SIZES)):
        tiny.append(read_of_events("6mer", 50000 + i, int(rng.integers(3, 41)), trim=int(rng.choice([2, 14]))))
        if i % 5 == 4:   # one anchor and then nothing: most diagonals are wider than a wave (the ring kernels' region)
            w = shaped_read("6mer", 60000 + i, int(rng.integers(90, 130)), int(rng.integers(150, 210)))
            wide.append(_with_anchors(w, [(w["ax"][0], w["ay"][0])]))
        else:
            wide.append(None)
    return tiny, wide


def g5_batch(n, with_wide=False, bad_at=None):
    tiny, wide = _g5_pool()
    jobs = [wide[i] if with_wide and wide[i] is not None else tiny[i] for i in range(n)]
    if bad_at is not None:   # a letter outside the alphabet: no planner takes this read, the host planner names the error
        j = tiny[bad_at]
        jobs[bad_at] = dict(j, ref=j["ref"][:3] + "N" + j["ref"][4:])
    return jobs


# ---- group 6: the split limit ---------------------------------------------------------------------------------------------------
G6_SPLIT = 2500                    # default_params(split=2500): an anchor-free rectangle of 50 x 50 stays, 50 x 51 splits the matrix
G6_RUN = 40


def g6_job(place, gy):
    """(x + 1, y + 1) anchors everywhere but for ONE anchor-free rectangle of 50 x gy: in front of the first anchor, between
    two anchors, or behind the last one"""
    n = G6_RUN
    if place == "front":
        pairs = [(50 + i, gy + i) for i in range(n)]
        lX, lY = 50 + n, gy + n
    elif place == "between":
        pairs = [(i, i) for i in range(10)] + [(10 + 50 + i, 10 + gy + i) for i in range(n)]
        lX, lY = 10 + 50 + n, 10 + gy + n
    else:
        pairs = [(i, i) for i in range(n)]
        lX, lY = n + 50, n + gy
    return [_with_anchors(shaped_read("6mer", 6000 + gy, lX, lY), pairs)]


def _ragged(build, ragged):
    fn, args = build
    return [dict(j, ragged=ragged) for j in fn(*args)]


def _remodel(build, model):
    """the same builder for another model's alphabet and k-mer length (the first argument of the builders that take one)"""
    fn, args = build
    return fn(model, *args[1:])


def jobs_of(case):
    fn, args = case.build
    return fn(*args)


DEFAULTS = ()
_T = [
    # 1. diagonal count on the stride
    Case("g1_diagonals_6mer", 1, "6mer", DEFAULTS, (g1_jobs, ("6mer",)), None, 0, None, 0),
    Case("g1_diagonals_5mer", 1, "5mer", DEFAULTS, (g1_jobs, ("5mer",)), None, 0, None, 0),
    # 2. path tables on the stride
    Case("g2_paths_cpg", 2, "cpg", DEFAULTS, (g2_jobs, ()), G2_AMBIG, 0, None, 0),
    # 3. anchor lists
    Case("g3_lists", 3, "6mer", DEFAULTS, (g3_lists, ("6mer",)), None, 0, None, 0),
    Case("g3_8191_8192_8193", 3, "6mer", DEFAULTS, (g3_big, G3_BIG), None, 0, None, 0),
    Case("g3_8193_alone", 3, "6mer", DEFAULTS, (g3_big, (8193,)), None, 0, None, 0),
    Case("g3_8193_own_anchors", 3, "6mer", DEFAULTS, (g3_big_own_anchors, ()), None, 0, None, 0),
    # 4. schedule
    Case("g4_defaults", 4, "6mer", DEFAULTS, (g4_reads, ("6mer",) + G4_EVENTS), None, 0, None, 0),
    Case("g4_tb0_md2", 4, "6mer", (("trace_back", 0), ("min_diags", 2)), (g4_reads, ("6mer", 400)), None, 0, None, 0),
    Case("g4_tb100_md102", 4, "6mer", (("trace_back", 100), ("min_diags", 102)), (g4_reads, ("6mer", 400)), None, 0, None, 0),
    Case("g4_tb1_md3", 4, "6mer", (("trace_back", 1), ("min_diags", 3)), (g4_reads, ("6mer", 400)), None, 0, None, 0),
    Case("g4_tb100_md3000", 4, "6mer", (("trace_back", 100), ("min_diags", 3000)), (g4_reads, ("6mer", 4000)), None, 0, None, 0),
    Case("g4_tb40_md64", 4, "6mer", (("trace_back", 40), ("min_diags", 64)), (g4_reads, ("6mer",) + G4_EVENTS), None, 0, None, 0),
    Case("g4_on_min_diags", 4, "6mer", (("min_diags", G4_MIN_DIAGS),), (g4_on_min_diags, ("6mer",)), None, 0, None, 0),
    # 5. batch size
    Case("g5_255", 5, "6mer", DEFAULTS, (g5_batch, (255,)), None, 0, None, 0),
    Case("g5_256", 5, "6mer", DEFAULTS, (g5_batch, (256,)), None, 0, None, 0),
    Case("g5_257", 5, "6mer", DEFAULTS, (g5_batch, (257,)), None, 0, None, 0),
    Case("g5_1023", 5, "6mer", DEFAULTS, (g5_batch, (1023,)), None, 0, None, 0),
    Case("g5_1024", 5, "6mer", DEFAULTS, (g5_batch, (1024,)), None, 0, None, 0),
    Case("g5_1025", 5, "6mer", DEFAULTS, (g5_batch, (1025, True)), None, 0, None, 0),
    Case("g5_2049", 5, "6mer", DEFAULTS, (g5_batch, (2049, True)), None, 0, None, 0),
    Case("g5_2049_passes", 5, "6mer", DEFAULTS, (g5_batch, (2049, True)), None, 0, (("SA_F_BUDGET_CELLPATHS", str(G5_BUDGET)),), 0),
    Case("g5_1025_bad_read_1024", 5, "6mer", DEFAULTS, (g5_batch, (1025, True, 1024)), None, 0, None, NOT_TAKEN),
    # 6. the split limit
    Case("g6_front_50x50", 6, "6mer", (("split", G6_SPLIT),), (g6_job, ("front", 50)), None, 0, None, 0),
    Case("g6_front_50x51", 6, "6mer", (("split", G6_SPLIT),), (g6_job, ("front", 51)), None, 0, None, NOT_TAKEN),
    Case("g6_between_50x50", 6, "6mer", (("split", G6_SPLIT),), (g6_job, ("between", 50)), None, 0, None, 0),
    Case("g6_between_50x51", 6, "6mer", (("split", G6_SPLIT),), (g6_job, ("between", 51)), None, 0, None, NOT_TAKEN),
    Case("g6_behind_50x50", 6, "6mer", (("split", G6_SPLIT),), (g6_job, ("behind", 50)), None, 0, None, 0),
    Case("g6_behind_50x51", 6, "6mer", (("split", G6_SPLIT),), (g6_job, ("behind", 51)), None, 0, None, NOT_TAKEN),
]

# 7. one pass of groups 1, 3 (without the reads of 8191 .. 8193 anchors) and 4 under the expectation pass's flag, under the R7.3
# model with the bundled HDP, and with the ragged-end booleans in all four combinations
G7_BASES = [c for c in _T if c.name in ("g1_diagonals_6mer", "g3_lists") or c.group == 4]
for _c in G7_BASES:
    _T.append(Case("g7_expect_" + _c.name, 7, "6mer", _c.params, _c.build, None, FLAG_EXPECT_INTERNAL, None, 0))
    _T.append(Case("g7_r73hdp_" + _c.name, 7, "r73hdp", _c.params, (_remodel, (_c.build, "r73hdp")), None, 0, None, 0))
    for _l in (0, 1):
        for _r in (0, 1):
            _T.append(Case("g7_ragged%d%d_%s" % (_l, _r, _c.name), 7, "6mer", _c.params, (_ragged, (_c.build, (_l, _r))), None, 0, None, 0))

CASES = {c.name: c for c in _T}
assert len(CASES) == len(_T)
# one batch of each of groups 1 to 5 that tests/test_gpu_dplan_edges.py aligns device-planned and host-planned; the first and
# the fourth also against the oracle -- and the 400-event read with trace_back = 0 (a traceback per diagonal that emits one diagonal,
# which the reference's debug build asserts against and its release build computes): what is planned there must also align
ALIGNED = ("g1_diagonals_6mer", "g2_paths_cpg", "g3_lists", "g4_tb40_md64", "g5_257", "g4_tb0_md2")
ALIGNED_AGAINST_ORACLE = ("g1_diagonals_6mer", "g4_tb40_md64", "g4_tb0_md2")
