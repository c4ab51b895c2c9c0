"""numpy restatements for the guide-alignment stage (include/signalalign_hip.h: sa_guide_align_batch; DESIGN.md, "Guide alignment"):

  banded      the banded local alignment with affine gaps, band by band as the rules state them; every neighbour is looked up by
              its matrix coordinates in the band that holds it (the device shifts registers instead), so the two agree only if
              both follow the rules.  The device's answer must equal this one bit for bit.
  unbanded    the optimal local affine score over the whole matrix, anti-diagonal by anti-diagonal (scores only)

plus the inputs the CPU and GPU tests share: the two real pairs and the 64 seeded synthetic pairs."""
import functools
import os

import numpy as np

NEG = -(1 << 30)
DEFAULTS = dict(match=2, mismatch=-4, gap_open=4, gap_extend=2, ambiguous=-1, band=128, min_read_fraction=0.5)
NO_ALIGNMENT, SHORT, BAND_EDGE, EMPTY, TRACE = 1, 2, 4, 8, 16

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_CODE = np.full(256, 4, dtype=np.int64)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _k
    _CODE[ord(_c.lower())] = _k


def codes(s):
    """0..3 for ACGT in either case, 4 for anything else"""
    return _CODE[np.frombuffer(s.encode("latin-1"), dtype=np.uint8)]


def _params(kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _border(i, j, n, m):
    inside = (i >= 0) & (i <= n) & (j >= 0) & (j <= m)
    return np.where(inside & ((i == 0) | (j == 0)), 0, NEG).astype(np.int64)


def _fetch(arr, ll_i_of_band, i_wanted):
    """value of the cell of row i_wanted in a band whose offset 0 lies on row ll_i_of_band; -inf outside the band"""
    off = ll_i_of_band - i_wanted
    ok = (off >= 0) & (off < len(arr))
    return np.where(ok, arr[np.clip(off, 0, len(arr) - 1)], NEG)


def banded(read, ref, diag=0, **kw):
    """-> dict(status, score, read_start, read_end, ref_start, ref_end, ops) with ops a list of (type, length) in read order"""
    p = _params(kw)
    W = int(p["band"])
    assert W % 64 == 0 and 64 <= W <= 256
    half = W // 2
    n, m = len(read), len(ref)
    out = dict(status=0, score=0, read_start=0, read_end=0, ref_start=0, ref_end=0, ops=[])
    if n == 0 or m == 0:
        out["status"] = EMPTY
        return out
    diag = min(max(int(diag), 0), m)
    rc_all, fc_all = codes(read), codes(ref)
    g_first, g_ext = p["gap_open"] + p["gap_extend"], p["gap_extend"]
    n_bands = n + m - diag
    o = np.arange(W, dtype=np.int64)
    ll_i, ll_j = half, diag - half
    lls = [ll_i]
    # band -1 (as if a right move led to band 0) and band 0: only row 0 and column 0 exist
    Hpp, ll_i2 = _border(ll_i - o, ll_j - 1 + o, n, m), ll_i
    Hp = _border(ll_i - o, ll_j + o, n, m)
    Ep, Fp = Hp.copy(), Hp.copy()
    ll_i1 = ll_i
    nibs = np.full((n_bands + 1, W), 3, dtype=np.uint8)
    best, best_b, best_o = 0, 0, 0
    downs = rights = 0
    prev_right = True
    for b in range(1, n_bands + 1):
        lo, hi = int(Hp[0]), int(Hp[W - 1])
        if downs == n:
            right = True
        elif diag + rights == m:
            right = False
        elif hi != lo:
            right = hi > lo
        else:
            right = not prev_right
        if right:
            ll_j += 1
            rights += 1
        else:
            ll_i += 1
            downs += 1
        i, j = ll_i - o, ll_j + o
        inside = (i >= 0) & (i <= n) & (j >= 0) & (j <= m)
        interior = inside & (i >= 1) & (j >= 1)
        lfH, lfE = _fetch(Hp, ll_i1, i), _fetch(Ep, ll_i1, i)             # (i, j-1)
        upH, upF = _fetch(Hp, ll_i1, i - 1), _fetch(Fp, ll_i1, i - 1)     # (i-1, j)
        dg = _fetch(Hpp, ll_i2, i - 1)                                    # (i-1, j-1)
        e_open, e_ext = lfH - g_first, lfE - g_ext
        f_open, f_ext = upH - g_first, upF - g_ext
        E = np.maximum(np.maximum(e_open, e_ext), 0)
        F = np.maximum(np.maximum(f_open, f_ext), 0)
        rc = rc_all[np.clip(i - 1, 0, n - 1)]
        fc = fc_all[np.clip(j - 1, 0, m - 1)]
        s = np.where((rc > 3) | (fc > 3), p["ambiguous"], np.where(rc == fc, p["match"], p["mismatch"]))
        d = dg + s
        H = np.maximum(np.maximum(np.maximum(d, E), F), 0)
        src = np.where(H <= 0, 3, np.where(H == d, 0, np.where(H == E, 1, 2)))
        nib = src | np.where(e_ext > e_open, 4, 0) | np.where(f_ext > f_open, 8, 0)
        off_val = np.where(inside, 0, NEG)
        H = np.where(interior, H, off_val)
        E = np.where(interior, E, off_val)
        F = np.where(interior, F, off_val)
        nibs[b] = np.where(interior, nib, 3)
        k = int(np.argmax(H))                                             # first maximum in offset order
        if H[k] > best:
            best, best_b, best_o = int(H[k]), b, k
        Hpp, ll_i2 = Hp, ll_i1
        Hp, Ep, Fp, ll_i1 = H, E, F, ll_i
        lls.append(ll_i)
        prev_right = right
    out["score"] = best
    if best <= 0:
        out["status"] = NO_ALIGNMENT
        return out
    ci = lls[best_b] - best_o
    cj = best_b + diag - ci
    out["read_end"], out["ref_end"] = ci, cj
    state, st, steps = 0, 0, []
    while True:
        b = ci + cj - diag
        if b < 0 or b > n_bands:
            st |= TRACE
            break
        off = lls[b] - ci
        if off < 0 or off >= W:
            st |= TRACE
            break
        if off == 0 or off == W - 1:
            st |= BAND_EDGE
        nib = int(nibs[b, off])
        if state == 0:
            src = nib & 3
            if src == 3:
                break
            if src == 1:
                state = 1
                continue
            if src == 2:
                state = 2
                continue
            steps.append(0)
            ci -= 1
            cj -= 1
        elif state == 1:
            steps.append(1)
            cj -= 1
            state = 1 if nib & 4 else 0
        else:
            steps.append(2)
            ci -= 1
            state = 2 if nib & 8 else 0
    out["read_start"], out["ref_start"] = ci, cj
    ops = []
    for t in reversed(steps):
        if ops and ops[-1][0] == t:
            ops[-1] = (t, ops[-1][1] + 1)
        else:
            ops.append((t, 1))
    out["ops"] = [] if st & TRACE else ops
    if (out["read_end"] - out["read_start"]) < p["min_read_fraction"] * float(n):
        st |= SHORT
    out["status"] = st
    return out


def unbanded(read, ref, **kw):
    """the optimal local affine score over the whole matrix"""
    p = _params(kw)
    n, m = len(read), len(ref)
    if n == 0 or m == 0:
        return 0
    rc, fc = codes(read), codes(ref)
    g_first, g_ext = p["gap_open"] + p["gap_extend"], p["gap_extend"]
    z = np.zeros(n + 1, dtype=np.int64)
    H1, E1, F1, H2 = z, z, z, z          # anti-diagonals d-1 and d-2, indexed by the row
    best = 0
    for d in range(2, n + m + 1):
        a, e = max(1, d - m), min(n, d - 1)            # rows of the interior cells of anti-diagonal d
        i = np.arange(a, e + 1)
        j = d - i
        E = np.maximum(np.maximum(H1[i] - g_first, E1[i] - g_ext), 0)
        F = np.maximum(np.maximum(H1[i - 1] - g_first, F1[i - 1] - g_ext), 0)
        x, y = rc[i - 1], fc[j - 1]
        s = np.where((x > 3) | (y > 3), p["ambiguous"], np.where(x == y, p["match"], p["mismatch"]))
        H = np.maximum(np.maximum(np.maximum(H2[i - 1] + s, E), F), 0)
        best = max(best, int(H.max()))
        Hn, En, Fn = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        Hn[a:e + 1], En[a:e + 1], Fn[a:e + 1] = H, E, F
        H2 = H1
        H1, E1, F1 = Hn, En, Fn
    return best


def match_pairs(read_start, ref_start, ops):
    """the (read index, reference index) pairs of an alignment's match operations"""
    pairs, i, j = set(), read_start, ref_start
    for t, ln in ops:
        if t == 0:
            pairs.update(zip(range(i, i + ln), range(j, j + ln)))
            i += ln
            j += ln
        elif t == 1:
            j += ln
        else:
            i += ln
    return pairs


def sam_match_pairs(cigar, ref_start):
    """the same for a SAM CIGAR string whose first aligned reference base is ref_start (0-based); S counts read bases"""
    import re
    pairs, i, j = set(), 0, ref_start
    for ln, op in re.findall(r"([0-9]+)([MIDNSHPX=])", cigar):
        ln = int(ln)
        if op in "M=X":
            pairs.update(zip(range(i, i + ln), range(j, j + ln)))
            i += ln
            j += ln
        elif op in "IS":
            i += ln
        elif op in "DN":
            j += ln
    return pairs


def reverse_complement(s):
    return s.translate(str.maketrans("ACGTacgt", "TGCAtgca"))[::-1]


@functools.lru_cache(maxsize=None)
def ecoli_pair():
    """(template read of r9p4_oneD.npRead, the 6817-base window of the reference's output, its one '?' read as A)"""
    z = np.load(os.path.join(GOLDEN, "expected", "reference_output_ecoli1d.npz"))
    window = str(z["window"]).replace("?", "A")
    with open(os.path.join(GOLDEN, "npReads", "r9p4_oneD.npRead")) as f:
        lines = f.read().split("\n")
    return lines[2].split()[0], window


@functools.lru_cache(maxsize=None)
def zymo_pair():
    """(2-D read of the bundled Zymo .npRead, ZymoRef.txt) as tests/golden/cigars/zymoC_lastz_anchors.json names them"""
    with open(os.path.join(GOLDEN, "npReads", "ZymoC_ch_1_file1.npRead")) as f:
        lines = f.read().split("\n")
    ref = open(os.path.join(GOLDEN, "npReads", "ZymoRef.txt")).read().split()[0].strip()
    return lines[1].split()[0], ref


def mutate(rng, seq, rate=0.12, max_indel=20):
    """substitutions, insertions and deletions in equal shares at `rate` per base; indel runs geometric, at most max_indel"""
    out, i = [], 0
    while i < len(seq):
        if rng.random() < rate:
            kind = rng.integers(3)
            ln = int(min(rng.geometric(0.5), max_indel))
            if kind == 0:
                out.append("ACGT"[("ACGT".index(seq[i]) + 1 + rng.integers(3)) % 4])
                i += 1
            elif kind == 1:
                out.extend("ACGT"[k] for k in rng.integers(4, size=ln))
            else:
                i += ln
        else:
            out.append(seq[i])
            i += 1
    return "".join(out)


@functools.lru_cache(maxsize=None)
def synthetic_pairs(count=64, seed=20240611):
    """(read, window) pairs: a random window of 200-1500 bases, the read a mutated copy of it (12 % errors, indel runs <= 20)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = []
    for _ in range(count):
        L = int(rng.integers(200, 1501))
        ref = "".join("ACGT"[k] for k in rng.integers(4, size=L))
        pairs.append((mutate(rng, ref), ref))
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def banded_cached(read, ref, diag=0, band=128):
    return banded(read, ref, diag, band=band)
