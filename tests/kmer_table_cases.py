"""Planted rows for the k-mer table (sa_kmer_table_add_rows): named cases that reach the branches of the top-N selection and of
the per-k-mer statistics (sa_train.hip) that rows out of a batch never reach.  Pure numpy, fixed seeds, no GPU.

A case is a k-mer id of its own (of the 6-mer model's 4096), its rows, and the N of the table it belongs to.  All cases of one
table lie in ONE run of rows: the free rows shuffled together and cut into three add_rows calls, rows that state a call put
into that call, rows that state a run ordinal put exactly there; the rows of strand 1 follow in a call of their own.  A row's
run ordinal is its index in the run, rows below min_prob included (add_rows skips them and still counts them).

What a case's name claims -- the radix level that settles its k-mer, the owner lane of k_kt_cut, the digit's offset within the
lane's 16 bins -- is proved by merge_trace(): the table's merges replayed call by call on the CPU with settle_shift
(tests/test_host_kmer_table_cases.py).  The GPU tests compare with top_n_arrays and ref.stats only.

Three k-mers cannot hold the same run ordinals in one table, so the three run-order ties of a table (need 2, 4 and 6 of 11
rows whose ordinals run from B - 4 to B + 6) sit at B, 2 B and 3 B: the key digits at and below B's own level are the same."""
import numpy as np

import kmer_training_ref as ref

N_KMERS = 4096
BIG = 1 << 20


class Table:
    """a run of rows (km, desc as float64, pu = posterior in 1e-6) cut into calls (strand, lo, hi), and its named cases"""

    def __init__(self, name, n, min_prob, km, desc, pu, calls, cases):
        self.name, self.n, self.min_prob = name, n, min_prob
        self.km, self.desc, self.pu = km, desc, pu
        self.calls, self.cases = calls, cases
        self.min_units = ref.min_units(min_prob)

    def prob(self):
        return self.pu / 1e6

    def strands(self):
        return sorted({c[0] for c in self.calls})

    def span(self, strand, n_calls=None):
        """[lo, hi) of the strand's rows: its calls are adjacent"""
        calls = [c for c in self.calls if c[0] == strand][:n_calls]
        assert all(a[2] == b[1] for a, b in zip(calls[:-1], calls[1:]))
        return calls[0][1], calls[-1][2]

    def kept(self, strand, n_calls=None):
        """{kmer_id: kept run ordinals in table order} after the strand's first n_calls calls (all by default)"""
        lo, hi = self.span(strand, n_calls)
        return ref.top_n_arrays(self.km[lo:hi], self.pu[lo:hi], self.n, self.min_units, first_ordinal=lo)

    def units(self, ordinal):
        return ref.units(ref.f6(self.desc[ordinal]))

    def expected_rows(self, strand, n_calls=None):
        """KMER_ROW-shaped tuples (kmer_id, prob_units, descaled_units, neg_zero, run) in the table's order"""
        out = []
        kept = self.kept(strand, n_calls)
        for km in sorted(kept):
            for o in kept[km].tolist():
                du, nz = self.units(o)
                out.append((km, int(self.pu[o]), du, nz, o))
        return out

    def kept_texts(self):
        """{("t" / "c", kmer_id): [(strand, kmer_id, desc text, prob text), ...]} as ref.table_lines reads it"""
        out = {}
        for s in self.strands():
            for km, ords in self.kept(s).items():
                out[("tc"[s], km)] = [("tc"[s], km, ref.f6(self.desc[o]), ref.f6(self.pu[o] / 1e6)) for o in ords.tolist()]
        return out

    def merge_trace(self, case):
        """settle_shift of the case's k-mer at every call of its strand: the candidates are the rows kept so far and the call's"""
        c = self.cases[case]
        out, kept = [], []
        for s, lo, hi in self.calls:
            if s != c["strand"]:
                continue
            new = lo + np.nonzero((self.km[lo:hi] == c["kmer"]) & (self.pu[lo:hi] >= self.min_units))[0]
            cand = kept + new.tolist()
            out.append(ref.settle_shift([ref.key(self.pu[o], o) for o in cand], self.n))
            kept = sorted(cand, key=lambda o: (-int(self.pu[o]), o))[:self.n]
        return out


class _Builder:
    def __init__(self, name, n, min_prob=0.0, seed=0):
        self.name, self.n, self.min_prob = name, n, min_prob
        self.rng = np.random.RandomState(seed)
        self.next_kmer = 3
        self.cases = {}
        self.free, self.in_call, self.pinned, self.strand1 = [], {0: [], 1: [], 2: []}, [], []

    def _rows(self, kmer, pu, desc):
        pu = np.asarray(pu, dtype=np.int64)
        assert pu.min() >= 0 and pu.max() <= 1000000
        if desc is None:   # event means to six decimals, as a real table holds them
            desc = self.rng.randint(40_000_000, 130_000_000, len(pu)) / 1e6
        return [(kmer, float(d), int(p)) for d, p in zip(np.asarray(desc, dtype=np.float64).tolist(), pu.tolist())]

    def case(self, name, pu, desc=None, shift=None, lane=None, offset=None, call=None, at=None, strand=0, kmer=None, **more):
        """shift: the levels one of which has to settle the k-mer at some merge (None: no claim); call: 0, 1 or 2, or one per
        row; at: run ordinal of the first row (the rows stay together, in this order)"""
        if kmer is None:
            kmer = self.next_kmer
            self.next_kmer += 7
        assert name not in self.cases and kmer < N_KMERS
        rows = self._rows(kmer, pu, desc)
        self.cases[name] = dict(kmer=kmer, strand=strand, shift=shift, lane=lane, offset=offset, n_rows=len(rows), **more)
        if strand == 1:
            self.strand1 += rows
        elif at is not None:
            self.pinned.append((at, rows))
        elif call is not None:
            for r, c in zip(rows, np.broadcast_to(call, len(rows)).tolist()):
                self.in_call[c].append(r)
        else:
            self.free += rows
        return kmer

    def more_rows(self, name, pu, desc=None, call=None):
        rows = self._rows(self.cases[name]["kmer"], pu, desc)
        self.cases[name]["n_rows"] += len(rows)
        if call is None:
            self.free += rows
        else:
            self.in_call[call] += rows

    def build(self):
        order = self.rng.permutation(len(self.free))
        edges = np.linspace(0, len(order), 4).astype(int)
        run, call_of = [], []
        for c in range(3):
            part = [self.free[i] for i in order[edges[c]:edges[c + 1]]] + self.in_call[c]
            # rows that state a call keep their own order, at random places among the call's free rows
            places = np.sort(self.rng.permutation(len(part))[:len(self.in_call[c])])
            mixed, stated, free = [], iter(self.in_call[c]), iter(part[:len(part) - len(self.in_call[c])])
            stated_at = set(places.tolist())
            for i in range(len(part)):
                mixed.append(next(stated) if i in stated_at else next(free))
            run += mixed
            call_of += [c] * len(mixed)
        for at, rows in sorted(self.pinned, key=lambda q: q[0]):
            assert 0 < at <= len(run), (self.name, at, len(run))
            c = call_of[at - 1] if at == len(run) else call_of[at]
            run[at:at] = rows
            call_of[at:at] = [c] * len(rows)
        calls, lo = [], 0
        call_of = np.array(call_of)
        for c in range(3):
            hi = lo + int((call_of == c).sum())
            calls.append((0, lo, hi))
            lo = hi
        assert lo == len(run) and all(b > a for _, a, b in calls)
        if self.strand1:
            run += self.strand1
            calls.append((1, lo, len(run)))
        return _table(self, run, calls)


def _table(b, run, calls):
    km = np.array([r[0] for r in run], dtype=np.int32)
    desc = np.array([r[1] for r in run], dtype=np.float64)
    pu = np.array([r[2] for r in run], dtype=np.int64)
    return Table(b.name, b.n, b.min_prob, km, desc, pu, calls, b.cases)


def _distinct_digits(digits, rng):
    """posteriors whose units >> 10 are the given digits, each with a low part of its own"""
    return [min(1000000, d * 1024 + int(r)) for d, r in zip(digits, rng.randint(0, 1024, len(digits)).tolist())]


def _shift50(b, name, n, cut_digit, n_below=3, **kw):
    """more than n posteriors in bins of their own at shift 50, the n-th largest in bin cut_digit"""
    above = [cut_digit + 1 + 2 * i for i in range(n - 1)]
    below = [cut_digit - 1 - i for i in range(n_below)]
    assert above == [] or above[-1] <= 976
    assert below[-1] >= 0
    pu = _distinct_digits(above + [cut_digit] + below, b.rng)
    if cut_digit == 976:
        pu[len(above)] = 1000000
    b.case(name, pu, shift=(50,), lane=cut_digit // 16, offset=cut_digit % 16, **kw)


def _shift40(b, name, n, digit):
    """n + 3 posteriors that share units >> 10 and differ below it"""
    low = b.rng.permutation(1024)[:n + 3]
    b.case(name, [digit * 1024 + int(q) for q in low], shift=(40,), call=1)   # (one call: the candidates are these rows)


def _counts(b, n):
    for c in (n - 1, n, n + 1):
        if c > 0:
            pu = b.rng.permutation(1000001)[:c]
            b.case("count_%d" % c, pu, shift=(50, 40) if c > n else (None,), call=0)


def _ties_at(b, base, level_shift):
    """11 rows tied at the cutoff posterior, ordinals B - 4 .. B + 6, preceded by the n - need rows that beat them"""
    for mult, need, shift in ((1, 2, 0), (2, 4, level_shift), (3, 6, 0)):
        beat = b.n - need
        pu = [900000 + 1024 * i for i in range(beat)] + [700000] * 11
        b.case("tie_%d_need%d" % (base, need), pu, shift=(shift,), at=mult * base - 4 - beat)


def _posterior_zero(b, n_pos, n_zero):
    """rows printed 0.000000 among others: n - n_pos of the n_zero are kept, the first in run order"""
    assert n_pos < b.n < n_pos + n_zero
    pu = list(b.rng.randint(1, 1000001, n_pos)) + [0] * n_zero
    b.case("posterior_zero", pu, shift=(10, 0), call=2, n_zero_kept=b.n - n_pos)


def _random_cases(b, count, n_rows):
    for i in range(count):
        grid = b.rng.randint(0, 1000001, 1 + b.rng.randint(1, n_rows))   # few distinct posteriors: ties at random cutoffs
        b.case("random_%d" % i, b.rng.choice(grid, n_rows))


def table_n1():
    b = _Builder("n1", 1, seed=101)
    _counts(b, 1)
    _shift50(b, "shift50_lane0_offset15", 1, 15, call=0)
    _shift50(b, "shift50_lane61_offset0", 1, 976, call=2)
    _shift40(b, "shift40", 1, 700)
    b.case("tie_2", [1000000] * 2, shift=(10, 0), call=1)
    b.case("tie_3_posterior_zero", [0] * 3, shift=(10, 0), call=1)
    for c in (1024, 1025, 5000):
        b.case("tie_%d" % c, [654321] * c, shift=(10, 0))
    return b.build()


def table_n2():
    b = _Builder("n2", 2, seed=102)
    _counts(b, 2)
    _shift50(b, "shift50_lane0_offset15", 2, 15, call=0)
    _shift50(b, "shift50_lane3_offset0", 2, 48, call=1)
    _shift40(b, "shift40", 2, 976 - 1)
    _posterior_zero(b, 1, 3)
    first = None
    for i in range(300):   # all in one call: 300 k-mers reach the run-order levels together and share the tie buffer
        km = b.case("open_%d" % i, [900000] * 5 + [950000], shift=(10, 0), call=1)
        first = km if first is None else first
    # both strands: strand 1 gets the very rows of a strand-0 case (other ordinals), other rows on a second strand-0 k-mer,
    # and a k-mer strand 0 does not have
    c = b.cases["shift50_lane0_offset15"]
    same = [r for r in b.in_call[0] if r[0] == c["kmer"]]
    b.case("strand1_same_rows", [r[2] for r in same], desc=[r[1] for r in same], strand=1, kmer=c["kmer"], shift=(50,))
    b.case("strand1_other_rows", [900000] * 4 + [123456], strand=1, kmer=first, shift=(10, 0))
    b.case("strand1_only", b.rng.randint(0, 1000001, 9), strand=1)
    return b.build()


def table_n7():
    b = _Builder("n7", 7, seed=107)
    _counts(b, 7)
    _shift50(b, "shift50_lane0_offset9", 7, 9, call=0)
    _shift50(b, "shift50_lane2_offset0", 7, 32, call=1)
    _shift50(b, "shift50_lane2_offset15", 7, 47, call=2)
    _shift40(b, "shift40", 7, 3)
    _posterior_zero(b, 4, 6)
    _random_cases(b, 40, 100)   # (4000 free rows: the run is long enough for the ties' ordinals)
    _ties_at(b, 1024, 10)
    # old rows against new: call 0 plants N rows; call 1 beats two of them and ties twice with the weakest old row left
    # (500000), which has the lower ordinal and stays; call 2 ties again, twice, and displaces nothing
    old = [900000, 800000, 700000, 600000, 500000, 400000, 300000]
    b.case("old_against_new", old, call=0, shift=(10, 0), weakest=500000)
    b.more_rows("old_against_new", [950000, 500000, 850000, 500000], call=1)
    b.more_rows("old_against_new", [500000, 500000], call=2)
    return b.build()


def table_n1025():
    b = _Builder("n1025", 1025, seed=1025)
    _counts(b, 1025)
    _posterior_zero(b, 1000, 100)
    b.case("tie_3000", [777777] * 3000, shift=(10, 0))
    _random_cases(b, 1, 3000)
    return b.build()


def table_far():
    """N = 7, min_prob 0.5: the ties at ordinals near 2^20, 2 * 2^20 and 3 * 2^20, reached through rows of posterior 0 that
    add_rows skips on the host and still counts"""
    b = _Builder("far", 7, min_prob=0.5, seed=120)
    _random_cases(b, 3, 30)
    _ties_at(b, BIG, 20)
    parts, calls, n = [b.free], [(0, 0, len(b.free))], len(b.free)
    for at, rows in sorted(b.pinned, key=lambda q: q[0]):
        assert at > n
        for part in (at - n, rows):   # a call of padding, then the case's rows in a call of their own
            calls.append((0, n, n + (part if isinstance(part, int) else len(part))))
            parts.append(part)
            n = calls[-1][2]
    km = np.concatenate([np.full(q, N_KMERS - 1) if isinstance(q, int) else [r[0] for r in q] for q in parts]).astype(np.int32)
    desc = np.concatenate([np.zeros(q) if isinstance(q, int) else [r[1] for r in q] for q in parts]).astype(np.float64)
    pu = np.concatenate([np.zeros(q) if isinstance(q, int) else [r[2] for r in q] for q in parts]).astype(np.int64)
    return Table(b.name, b.n, b.min_prob, km, desc, pu, calls, b.cases)


SELECTION = {"n1": table_n1, "n2": table_n2, "n7": table_n7, "n1025": table_n1025, "far": table_far}
_cache = {}


def selection_table(name):
    if name not in _cache:
        _cache[name] = SELECTION[name]()
    return _cache[name]


# ---- the statistics table: N = 2^20, min_prob 0, every row kept --------------------------------------------------------------
LIMIT = float(np.nextafter(2147.483648, 0))   # the largest accepted magnitude: "%f" rounds it to 2147.483648, 2^31 units
LIMIT_UNITS = 1 << 31
CARRY_CASES = ("limit_5", "limit_257", "limit_4097")


def _of_units(u):
    u = np.asarray(u, dtype=np.int64)
    return u / 1e6, u, np.zeros(len(u), dtype=np.int64)


def _limits(signs):
    signs = np.asarray(signs, dtype=np.int64)
    return signs * LIMIT, signs * LIMIT_UNITS, np.zeros(len(signs), dtype=np.int64)


def statistics_cases():
    """{case name: (float64 values, planted units, planted negative-zero flags)}, in the order the k-mer ids are given out"""
    rng = np.random.RandomState(77)
    v = {}
    for n in (1, 2, 3, 4, 255, 256, 257, 513, 5000):   # symmetric about 0, both signs, to six decimals
        x = rng.randint(1, 150_000_000, n // 2)
        v["count_%d" % n] = _of_units(np.concatenate([x, -x, [-61250000] if n == 1 else [0] * (n % 2)]))
    v["all_equal"] = _of_units([-81250000] * 300)
    v["two_values"] = _of_units([71000001] * 128 + [79500000] * 128)      # the two middle values differ: a median in half units
    v["lowest_byte_only"] = _of_units(0x04A3B200 + rng.permutation(256)[:200])   # one occupied bin in the upper seven passes
    v["sign_only"] = _of_units([66123457, -66123457] * 50)
    v["limit_5"] = _limits([1] * 5)
    v["limit_257"] = _limits(np.where(np.arange(257) % 2 == 0, 1, -1))
    v["limit_4097"] = _limits([-1] * 4097)
    mixed, small = _limits([1, -1] * 500), _of_units([3])                 # S = 3 units, Q = 1000 * 2^62 + 9
    v["limit_mixed"] = tuple(np.concatenate([a, c]) for a, c in zip(mixed, small))
    v["zero_units"] = (np.array([-0.0, -1e-9, 4e-7]), np.zeros(3, dtype=np.int64), np.array([1, 1, 0]))
    v["mad_middle_differs"] = _of_units([0, 1, 3, 10])
    return v


class StatisticsTable:
    def __init__(self):
        rng = np.random.RandomState(78)
        self.cases = statistics_cases()
        self.kmer = {name: 5 + 11 * i for i, name in enumerate(self.cases)}
        km = np.concatenate([np.full(len(c[0]), self.kmer[name], dtype=np.int32) for name, c in self.cases.items()])
        desc = np.concatenate([c[0] for c in self.cases.values()])
        pu = rng.randint(0, 1000001, len(km)).astype(np.int64)
        order = rng.permutation(len(km))
        edges = np.linspace(0, len(km), 4).astype(int)
        calls = [(0, int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
        self.table = Table("statistics", BIG, 0.0, km[order], desc[order], pu[order], calls, {})

    def units(self, name):
        """the planted units of a case's rows"""
        return self.cases[name][1].tolist()


def statistics_table():
    if "statistics" not in _cache:
        _cache["statistics"] = StatisticsTable()
    return _cache["statistics"]
