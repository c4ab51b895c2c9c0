"""sa_guide_locate_batch on the GPU against tests/locate_ref.py's restatement: every field of sa_locate_result_t is compared.
The shared reference and its restated index are built once (locate_ref.shared_reference / shared_index)."""
import functools

import numpy as np
import pytest

import signalalign_amd as sa

import guide_ref as g
import locate_ref as L

pytestmark = pytest.mark.gpu


class Ref:
    """a reference on the device and its restated index"""

    def __init__(self, seqs, names=None):
        self.seqs = list(seqs)
        self.names = list(names) if names else ["c%d" % i for i in range(len(self.seqs))]
        self.dev = sa.ref_index_build(self.names, self.seqs, device=0)
        self.ref = L.build_index(self.seqs)


def check(R, reads, **params):
    """one batch on the device, every read against the restatement; returns the device's results"""
    got = sa.guide_locate_batch(R.dev, list(reads), sa.locate_params(**params) if params else None)
    assert len(got) == len(reads)
    for k, (read, res) in enumerate(zip(reads, got)):
        exp = L.locate(R.ref, read, **params)
        assert res == exp, (k, len(read), params, res, exp)
    return got


@pytest.fixture(scope="module")
def shared():
    R = Ref(L.shared_reference(), L.NAMES)
    info = sa.ref_index_info(R.dev)
    assert info["device"] == 0 and info["device_bytes"] == 8 * info["n_entries"] + 4 * ((1 << info["q"]) + 1) + 4 * 4
    return R


UNIT_COPIES = 512


@functools.lru_cache(maxsize=None)
def unit_parts():
    rng = np.random.Generator(np.random.PCG64(40))
    return L.rand_seq(rng, 40), L.rand_seq(rng, 600)


@pytest.fixture(scope="module")
def units():
    """a 40-base unit 512 times, then 600 unique bases: a 15-mer of the unit that starts at phase 0..25 of it occurs 512 times"""
    unit, tail = unit_parts()
    return Ref([unit * UNIT_COPIES + tail])


def test_the_real_reads(shared):
    read, _ = g.ecoli_pair()
    got = check(shared, [read, g.reverse_complement(read)])
    assert [(r["status"], r["contig"], r["reverse"]) for r in got] == [(0, 0, 0), (0, 0, 1)]
    assert abs(got[0]["pos"] - (L.WINDOW_AT - 42)) <= 64 and got[0]["seeds"] == 2000 - 14 and got[0]["votes"] >= 400
    # the bundled Zymo read against its bundled reference as a one-contig reference
    zread, zref = g.zymo_pair()
    Z = Ref([zref], ["zymo"])
    z = check(Z, [zread])[0]
    assert z["status"] == 0 and z["contig"] == 0 and z["votes"] >= 8


def test_read_lengths_around_a_seed_a_wave_and_read_bases(shared):
    read, _ = g.ecoli_pair()
    lens = (0, 14, 15, 16, 63, 64, 65, 255, 256, 257, 1999, 2000, 2001, 2500)
    got = check(shared, [read[:n] for n in lens])
    for n, r in zip(lens, got):
        assert (r["status"] == sa.LOCATE_EMPTY) == (n < 15), n
        assert r["seeds"] == max(min(n, 2000) - 14, 0), n          # the seed count stops growing at read_bases
    assert got[-1]["status"] == 0 and got[-1] == got[-2] == got[-3]
    assert got[-4] != got[-3]                                       # 1999 bases: one seed fewer
    # another read_bases: the seeds stop there
    r = check(shared, [read], read_bases=512)[0]
    assert r["seeds"] == 512 - 14 and r["status"] == 0
    assert check(shared, [read], read_bases=2048)[0]["seeds"] == 2048 - 14
    assert check(shared, [read[:300]], read_bases=15)[0]["seeds"] == 1


@pytest.mark.parametrize("max_hits", [1024, 8192])
def test_hit_counts_around_the_padding_and_the_cap(units, max_hits):
    """s seeds of the unit give 512 hits each, x seeds of the unique tail one each: s * 512 + x hits exactly"""
    unit, tail = unit_parts()
    s = max_hits // UNIT_COPIES - 1
    for x in (UNIT_COPIES - 1, UNIT_COPIES, UNIT_COPIES + 1):
        read = (unit * 2)[:14 + s] + "N" + tail[20:20 + 14 + x]
        r = check(units, [read], max_occ=UNIT_COPIES, max_hits=max_hits)[0]
        total = s * UNIT_COPIES + x
        assert r["seeds"] == s + x and r["hits"] == min(total, max_hits) and r["reverse"] == 0, (x, r)
        assert bool(r["status"] & sa.LOCATE_OVERFLOW) == (total > max_hits), (x, r)
    # far above the cap: only the unit's seeds fit
    read = (unit * 2)[:14 + 26]
    r = check(units, [read], max_occ=UNIT_COPIES, max_hits=max_hits)[0]
    assert r["hits"] == max_hits and r["status"] & sa.LOCATE_OVERFLOW


def test_no_hit_one_hit_and_a_few(units):
    unit, tail = unit_parts()
    rng = np.random.Generator(np.random.PCG64(41))
    got = check(units, [L.rand_seq(rng, 700), tail[100:115], tail[100:116], tail[100:117], tail[100:122], tail[100:123]])
    assert [r["hits"] for r in got] == [0, 1, 2, 3, 8, 9]            # 1, 2, 4, 8 and 16 sorted keys
    assert [r["status"] for r in got] == [sa.LOCATE_NONE] * 4 + [0, 0] and got[0]["votes"] == 0 and got[0]["contig"] == -1
    assert got[4]["pos"] == 40 * UNIT_COPIES + 100


def test_max_occ_edges(units):
    unit, tail = unit_parts()
    read = (unit * 2)[:14 + 20]                                      # 20 seeds of 512 occurrences each
    r = check(units, [read], max_occ=UNIT_COPIES)[0]
    assert r["hits"] == 8192 and r["repetitive"] == 0
    r = check(units, [read], max_occ=UNIT_COPIES - 1)[0]
    assert r["hits"] == 0 and r["repetitive"] == 20 and r["status"] == sa.LOCATE_NONE
    # the unit 33 times: a 15-mer occurs 33 times from phases 0..25, 32 times from phases 26..39
    R33 = Ref([unit * 33])
    read = unit * 2
    r = check(R33, [read], max_occ=32)[0]
    assert r["seeds"] == 66 and r["repetitive"] == 26 * 2 and r["hits"] == 14 * 32
    r = check(R33, [read], max_occ=33)[0]
    assert r["repetitive"] == 0 and r["hits"] == 52 * 33 + 14 * 32
    # two copies of everything: max_occ = 1 lets nothing vote, 2 everything
    rng = np.random.Generator(np.random.PCG64(42))
    s = L.rand_seq(rng, 400)
    twin = Ref([s, "ACGT" * 10, s])
    r = check(twin, [s[50:250]], max_occ=1)[0]
    assert r["repetitive"] == 200 - 14 and r["hits"] == 0
    r = check(twin, [s[50:250]], max_occ=2)[0]
    assert r["repetitive"] == 0 and r["hits"] == 2 * (200 - 14)


def test_tie_rules():
    rng = np.random.Generator(np.random.PCG64(43))
    s, x = L.rand_seq(rng, 500), L.rand_seq(rng, 150)
    # two loci with equal votes: the lower key
    twin = Ref([s, s])
    r = check(twin, [s[100:300]])[0]
    assert (r["contig"], r["pos"], r["votes"], r["second_votes"]) == (0, 100, 186, 186) and r["status"] == sa.LOCATE_AMBIGUOUS
    # equal votes on both strands: forward
    both = Ref([s, g.reverse_complement(s)])
    r = check(both, [s[100:300]])[0]
    assert (r["contig"], r["reverse"], r["pos"], r["votes"]) == (0, 0, 100, 186) and r["status"] == 0
    r = check(both, [g.reverse_complement(s[100:300])])[0]
    assert (r["contig"], r["reverse"], r["pos"]) == (1, 0, 200)
    # a read that is its own reverse complement
    pal = x + g.reverse_complement(x)
    assert pal == g.reverse_complement(pal)
    P = Ref([s[:200] + pal + s[200:]])
    r = check(P, [pal])[0]
    assert (r["reverse"], r["pos"], r["status"]) == (0, 200, 0) and r["votes"] == 300 - 14


def test_anchor_of_a_clipped_read_falls_in_the_neighbouring_contig(shared):
    """1200 bases that are nowhere, then contig 1's first 300: the diagonal starts 1200 before contig 1, the anchor (750 further)
    still lies in contig 0 -- the contig rule as stated names contig 0, and the position runs past its end"""
    rng = np.random.Generator(np.random.PCG64(44))
    read = L.rand_seq(rng, 1200) + L.shared_reference()[1][:300]
    r = check(shared, [read])[0]
    assert r["status"] == 0 and (r["contig"], r["reverse"], r["pos"]) == (0, 0, 120000 - 1200)
    # the same read's reverse complement
    r = check(shared, [g.reverse_complement(read)])[0]
    assert r["status"] == 0 and (r["contig"], r["reverse"]) == (0, 1) and r["pos"] == 120000 + 299


def test_letters_outside_acgt_and_lower_case(shared):
    read, _ = g.ecoli_pair()
    piece = read[:900]
    holes = list(piece)
    for i in range(7, 900, 50):
        holes[i] = "N"
    mixed = "".join(holes)
    got = check(shared, [piece.lower(), mixed, mixed.lower()[:450] + mixed[450:], "N" * 500, "N" * 14 + piece[:15], "E" + piece[:100]])
    assert got[0] == check(shared, [piece])[0] and got[1] == got[2]
    assert got[1]["seeds"] == 886 - 8 - 17 * 15 and got[1]["status"] == 0          # the first N takes 8 seeds, the others 15
    assert got[3]["seeds"] == 0 and got[3]["status"] == sa.LOCATE_NONE and got[4]["seeds"] == 1 and got[5]["seeds"] == 86


def mixed_batch():
    read, _ = g.ecoli_pair()
    rng = np.random.Generator(np.random.PCG64(45))
    reads = [r[0] for r in L.synthetic_reads()[:24]]
    reads += [read, g.reverse_complement(read), "", "ACGT", L.rand_seq(rng, 900), "N" * 40, read[:15], read[3000:3600],
              g.reverse_complement(read[2000:2100])]
    assert len(reads) == 33
    return reads


def test_a_batch_equals_its_reads_one_at_a_time_and_survives_release_and_growth(shared):
    reads = mixed_batch()
    batch = check(shared, reads)
    for k, read in enumerate(reads):
        assert sa.guide_locate_batch(shared.dev, [read])[0] == batch[k], k
    sa.locate_release()
    assert sa.guide_locate_batch(shared.dev, reads) == batch
    sa.locate_release()
    read, _ = g.ecoli_pair()
    longer = [read[i:i + 2000] for i in range(0, 4000, 50)] + reads
    assert sa.guide_locate_batch(shared.dev, reads[:3]) == batch[:3]            # small scratch first ...
    assert sa.guide_locate_batch(shared.dev, longer)[len(longer) - len(reads):] == batch          # ... grown by a longer batch
    assert sa.guide_locate_batch(shared.dev, reads) == batch
    assert sa.guide_locate_batch(shared.dev, []) == []


def test_two_indexes_answer_independently(shared):
    read, window = g.ecoli_pair()
    other = Ref([L.shared_reference()[2], window], ["small", "win"])
    for _ in range(2):
        a = check(shared, [read, read[::-1]])
        b = check(other, [read, L.shared_reference()[2][500:900]])
        assert (a[0]["contig"], b[0]["contig"], b[1]["contig"]) == (0, 1, 0) and b[0]["pos"] != a[0]["pos"]
    other.dev.close()
    assert check(shared, [read])[0] == a[0]


def test_the_synthetic_reads_equal_the_restatement(shared):
    reads = L.synthetic_reads()
    got = sa.guide_locate_batch(shared.dev, [r[0] for r in reads])
    for k, (r, res) in enumerate(zip(reads, got)):
        assert res == L.located(r[0]), k
