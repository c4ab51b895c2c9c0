"""Locating a read in a whole reference, restated in numpy: the index layout of sa_ref_index_t and the rules of
sa_guide_locate_batch ("Locating a read in a whole reference").  No device, no library: the index built by the
library and the device's answers are compared with this field for field.  Also the seeded reference the locate tests share."""
import functools

import numpy as np

import guide_ref as g

K = 15
NONE, AMBIGUOUS, OVERFLOW, EMPTY = 1, 2, 4, 8
DEFAULTS = dict(read_bases=2000, max_occ=32, span=128, min_votes=8, max_hits=8192)
FIELDS = ("status", "contig", "reverse", "pos", "key", "votes", "second_votes", "hits", "seeds", "repetitive")

_CODE = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def encode(seq):
    """0..3 for ACGT in either case, 4 for anything else"""
    return _CODE[np.frombuffer(seq.encode("latin-1"), dtype=np.uint8)]


def kmers(codes):
    """for every p in [0, len - K]: (all K letters are of ACGT, the k-mer's code, the code of its reverse complement); the first
    letter is the most significant pair of bits, as sa_guide.c encodes"""
    n = len(codes) - K + 1
    if n <= 0:
        z = np.zeros(0, dtype=np.int64)
        return z.astype(bool), z, z
    ok = np.ones(n, dtype=bool)
    fwd, rev = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(K):
        c = codes[i:i + n]
        ok &= c < 4
        fwd |= (c & 3) << (2 * (K - 1 - i))
        rev |= (3 - (c & 3)) << (2 * i)
    return ok, fwd, rev


def table_bits(n_entries):
    q = 16
    while q < 26 and (1 << q) < n_entries:
        q += 2
    return q


def build_index(seqs):
    """dict(codes uint32, pos int32, table int32 of 2^q + 1, q, starts int64 of n_contigs + 1, total)"""
    starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    cs, ps = [], []
    for s, at in zip(seqs, starts):
        ok, fwd, _ = kmers(encode(s))
        cs.append(fwd[ok])
        ps.append(np.nonzero(ok)[0] + at)
    codes, pos = np.concatenate(cs), np.concatenate(ps)
    order = np.argsort(codes, kind="stable")          # positions stay ascending inside a code
    codes, pos = codes[order], pos[order]
    q = table_bits(len(codes))
    table = np.searchsorted(codes >> (2 * K - q), np.arange((1 << q) + 1), side="left")
    return dict(codes=codes.astype(np.uint32), pos=pos.astype(np.int32), table=table.astype(np.int32), q=q, starts=starts,
                total=int(starts[-1]))


def _strand(index, seed_pos, seed_codes, sign, P):
    """one strand's vote: (votes, key, second_votes, kept hits, repetitive seeds, hits were dropped)"""
    codes, pos = index["codes"], index["pos"].astype(np.int64)
    lo, hi = np.searchsorted(codes, seed_codes, side="left"), np.searchsorted(codes, seed_codes, side="right")
    occ = hi - lo
    repetitive = int(np.count_nonzero(occ > P["max_occ"]))
    use = (occ > 0) & (occ <= P["max_occ"])
    lo, occ, p = lo[use], occ[use], seed_pos[use]
    total = int(occ.sum())
    first = np.cumsum(occ) - occ                       # seed by seed in read order, ascending r inside a seed
    entry = np.repeat(lo - first, occ) + np.arange(total)
    keys = pos[entry] + sign * np.repeat(p, occ)       # forward r - p, reverse r + p
    keys = np.sort(keys[:P["max_hits"]])
    if len(keys) == 0:
        return 0, 0, 0, 0, repetitive, False
    c = np.searchsorted(keys, keys + P["span"], side="left") - np.searchsorted(keys, keys, side="left")
    best = int(np.argmax(c))                           # the first maximum
    votes = int(c[best])
    key = int(keys[best + (votes - 1) // 2])
    far = (keys < keys[best] - P["span"]) | (keys >= keys[best] + 2 * P["span"])
    second = int(c[far].max()) if far.any() else 0
    return votes, key, second, len(keys), repetitive, total > P["max_hits"]


def locate(index, read, **params):
    P = dict(DEFAULTS, **params)
    out = dict.fromkeys(FIELDS, 0)
    out["contig"] = -1
    if len(read) < K:
        out["status"] = EMPTY
        return out
    bases = min(len(read), P["read_bases"])
    ok, fwd, rev = kmers(encode(read[:bases]))
    seed_pos = np.nonzero(ok)[0]
    f = _strand(index, seed_pos, fwd[ok], -1, P)
    r = _strand(index, seed_pos, rev[ok], +1, P)
    reverse = r[0] > f[0]
    votes, key, second, hits, repetitive, _ = r if reverse else f
    status = OVERFLOW if (f[5] or r[5]) else 0
    out.update(reverse=int(reverse), key=key, votes=votes, second_votes=second, hits=hits, seeds=len(seed_pos), repetitive=repetitive)
    if votes < P["min_votes"]:
        out["status"] = status | NONE
        return out
    if 4 * second >= 3 * votes:
        status |= AMBIGUOUS
    half = bases // 2
    anchor = key + K - 1 - half if reverse else key + half
    anchor = min(max(anchor, 0), index["total"] - 1)
    contig = int(np.searchsorted(index["starts"], anchor, side="right")) - 1       # the last contig that starts at or before it
    contig = min(contig, len(index["starts"]) - 2)
    out.update(status=status, contig=contig, pos=(key + K - 1 if reverse else key) - int(index["starts"][contig]))
    return out


def window(index, res, read_len, band):
    """[start, end) in the contig's coordinates, clipped to the contig"""
    ln = int(index["starts"][res["contig"] + 1] - index["starts"][res["contig"]])
    pos, ext = res["pos"], read_len + read_len // 4 + band
    lo, hi = (pos + 1 - ext, pos + 1 + band) if res["reverse"] else (pos - band, pos + ext)
    return max(lo, 0), min(hi, ln)


# ---- the reference the locate tests share -------------------------------------------------------------------------------------
NAMES = ("ctgA", "ctgB", "ctgC")
WINDOW_AT = 40000                  # of contig 0: where the E. coli window is planted
REPEAT_AT, REPEAT_LEN = 90000, 3000
REPEAT_COPIES = ((1, 10000), (1, 40000))


def rand_seq(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(4, size=n))


@functools.lru_cache(maxsize=None)
def shared_reference(seed=20240921):
    """three contigs of 120 000, 60 000 and 20 000 random bases; contig 0 holds the bundled E. coli window and a 3000-base stretch
    that contig 1 holds twice more.  (The seed is one whose bases around the planted window do not extend the read's alignment
    past it by chance matches: with 20240917 the alignment ran one base over.)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    a, b, c = (rand_seq(rng, n) for n in (120000, 60000, 20000))
    _, win = g.ecoli_pair()
    a = a[:WINDOW_AT] + win + a[WINDOW_AT + len(win):]
    rep = a[REPEAT_AT:REPEAT_AT + REPEAT_LEN]
    for _, at in REPEAT_COPIES:
        b = b[:at] + rep + b[at + REPEAT_LEN:]
    assert (len(a), len(b), len(c)) == (120000, 60000, 20000)
    return (a, b, c)


@functools.lru_cache(maxsize=None)
def shared_index():
    return build_index(shared_reference())


@functools.lru_cache(maxsize=None)
def synthetic_reads(count=64, seed=20240918):
    """(read, contig, reverse, contig coordinate of read base 0, wholly inside a copy of the repeat) of reads of 200-1500 bases
    with 12 % errors, alternating strands; reads 10 and 41 are drawn inside a copy of the repeat, the others clear of every copy"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref = shared_reference()
    copies = ((0, REPEAT_AT),) + REPEAT_COPIES
    out = []
    for k in range(count):
        n = int(rng.integers(200, 1501))
        inside = k in (10, 41)
        while True:
            if inside:
                ci, at = copies[k % 3]
                a = at + int(rng.integers(0, REPEAT_LEN - n + 1))
            else:
                ci = int(rng.integers(3))
                a = int(rng.integers(0, len(ref[ci]) - n + 1))
            if inside or all(c != ci or a + n <= at or a >= at + REPEAT_LEN for c, at in copies):
                break
        piece = g.mutate(rng, ref[ci][a:a + n])
        reverse = k % 2 == 1
        out.append((g.reverse_complement(piece) if reverse else piece, ci, reverse, a + n - 1 if reverse else a, inside))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def located(read, **params):
    """the restatement's answer on the shared reference, computed once per (read, parameters)"""
    return locate(shared_index(), read, **params)
