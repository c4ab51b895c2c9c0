"""The locate stage without a GPU: the library's reference index against the numpy restatement (tests/locate_ref.py) bit for bit,
the restatement's own answers on the shared reference, the window handed to the guide stage, the argument checks, the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import guide_ref as g
import locate_ref as L
import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")


def same_index(seqs, names=None):
    """the library's host-only index of `seqs` equals the restatement's; returns the restatement's"""
    names = names or ["c%d" % i for i in range(len(seqs))]
    ix = sa.ref_index_build(names, seqs, device=-1)
    got, exp, info = sa.ref_index_entries(ix), L.build_index(seqs), sa.ref_index_info(ix)
    assert got["q"] == exp["q"] and got["total"] == exp["total"] == info["total_bases"]
    for f in ("codes", "pos", "table", "starts"):
        assert got[f].dtype == exp[f].dtype and np.array_equal(got[f], exp[f]), f
    assert info["n_entries"] == len(exp["codes"]) and info["n_contigs"] == len(seqs) and info["device"] == -1
    assert info["device_bytes"] == 0 and info["host_bytes"] == 8 * len(exp["codes"]) + 4 * len(exp["table"]) + 8 * len(exp["starts"])
    assert len(exp["table"]) == (1 << exp["q"]) + 1 and exp["table"][0] == 0 and exp["table"][-1] == len(exp["codes"])
    for i, s in enumerate(seqs):
        assert ix.contig(i) == (names[i], int(exp["starts"][i]), len(s))
    ix.close()
    return exp


def test_index_of_the_shared_reference_equals_the_restatement():
    exp = same_index(list(L.shared_reference()), list(L.NAMES))
    assert exp["q"] == 18 and len(exp["codes"]) == 200000 - 3 * 14          # 2^18 >= 199 958 > 2^16
    # sorted by (code, pos)
    order = np.lexsort((exp["pos"], exp["codes"]))
    assert np.array_equal(order, np.arange(len(order)))


def test_index_edges():
    rng = np.random.Generator(np.random.PCG64(5))
    for n, entries in ((14, 0), (15, 1), (16, 2)):
        assert len(same_index([L.rand_seq(rng, n)])["codes"]) == entries
    s = list(L.rand_seq(rng, 600))
    s[14::15] = "N" * len(s[14::15])                                       # an N every 15th base: no 15 letters in a row
    assert len(same_index(["".join(s)])["codes"]) == 0
    s = L.rand_seq(rng, 300)
    low = same_index([s.lower()[:150] + s[150:]])
    assert np.array_equal(low["codes"], L.build_index([s])["codes"])
    # a k-mer that would span a boundary: two halves of one sequence give 14 entries fewer than the whole
    assert len(same_index([s[:150], s[150:]])["codes"]) == len(L.build_index([s])["codes"]) - 14
    # methyl letters break a k-mer as N does
    assert len(same_index([s[:100] + "E" + s[101:]])["codes"]) == 300 - 14 - 15
    # two contigs with identical content: every code twice, positions ascending
    twin = same_index([s, s])
    assert np.array_equal(twin["codes"][0::2], twin["codes"][1::2]) and np.all(twin["pos"][1::2] - twin["pos"][0::2] == 300)
    # an empty contig between two others
    same_index([s[:100], "", s[100:]])


def test_index_from_a_fasta(tmp_path):
    ref = L.shared_reference()
    path = str(tmp_path / "ref.fa")
    with open(path, "w") as f:
        for name, s in zip(L.NAMES, ref):
            f.write(">%s some description\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    ix = sa.ref_index_build_fasta(path, device=-1)
    got, exp = sa.ref_index_entries(ix), L.shared_index()
    for f in ("codes", "pos", "table", "starts"):
        assert np.array_equal(got[f], exp[f]), f
    assert [ix.contig(i)[0] for i in range(3)] == list(L.NAMES)
    with pytest.raises(sa.SaError) as e:
        sa.ref_index_build_fasta(str(tmp_path / "absent.fa"), device=-1)
    assert e.value.code == -6


def test_restatement_locates_the_synthetic_reads():
    """On the restatement alone: every read drawn clear of the repeat is located on its contig and strand within 200 of the
    truth with status 0, every read drawn inside a copy of the repeat is ambiguous."""
    reads = L.synthetic_reads()
    assert len(reads) == 64 and all(200 <= len(r[0]) <= 1800 for r in reads)
    n_inside = 0
    for k, (read, contig, reverse, pos, inside) in enumerate(reads):
        r = L.located(read)
        print(k, len(read), contig, reverse, pos, inside, r)
        if inside:
            n_inside += 1
            assert r["status"] & L.AMBIGUOUS and r["second_votes"] == r["votes"], (k, r)
        else:
            assert r["status"] == 0 and r["contig"] == contig and r["reverse"] == int(reverse) and abs(r["pos"] - pos) <= 200, (k, r)
    assert n_inside == 2


@pytest.mark.parametrize("band", [64, 128, 256])
def test_window_holds_the_aligned_interval_of_the_ecoli_read(band):
    read, window = g.ecoli_pair()
    aligned = g.banded_cached(read, window, 0, 128)
    lo, hi = L.WINDOW_AT + aligned["ref_start"], L.WINDOW_AT + aligned["ref_end"]
    ix = sa.ref_index_build(list(L.NAMES), list(L.shared_reference()), device=-1)
    for rd, reverse in ((read, 0), (g.reverse_complement(read), 1)):
        r = L.located(rd)
        assert r["status"] == 0 and r["contig"] == 0 and r["reverse"] == reverse
        a, b = sa.locate_window(ix, r, len(rd), band)
        assert (a, b) == L.window(L.shared_index(), r, len(rd), band)
        assert a <= lo and hi <= b and b - a <= len(rd) + len(rd) // 4 + 2 * band
    # clipped to the contig, and refused without a location
    r = dict(L.located(read), pos=-50)
    assert sa.locate_window(ix, r, len(read), band) == (0, -50 + len(read) + len(read) // 4 + band)
    r = dict(L.located(read), pos=119000)
    assert sa.locate_window(ix, r, len(read), band) == (119000 - band, 120000)
    for bad in (dict(L.located(read), contig=-1), dict(L.located(read), contig=3), dict(L.located(read), pos=130000)):
        with pytest.raises(sa.SaError) as e:
            sa.locate_window(ix, bad, len(read), band)
        assert e.value.code == -1


def test_argument_checks():
    with pytest.raises(sa.SaError) as e:
        sa.ref_index_build([], [], device=-1)
    assert e.value.code == -1
    with pytest.raises(sa.SaError) as e:
        sa.ref_index_build(["a"], [None], device=-1, lens=[5])
    assert e.value.code == -1
    with pytest.raises(sa.SaError) as e:
        sa.ref_index_build(["a"], ["ACGT"], device=-1, lens=[-1])
    assert e.value.code == -1
    assert sa.lib().sa_ref_index_build(None, None, None, None, 1, -1) == -1
    # too long in all: refused on the lengths, before a sequence is read
    for lens in ([2 ** 31 - 2 ** 16], [2 ** 30, 2 ** 30 - 2 ** 16], [2 ** 40]):
        with pytest.raises(sa.SaError) as e:
            sa.ref_index_build(["c%d" % i for i in range(len(lens))], ["ACGT"] * len(lens), device=-1, lens=lens)
        assert e.value.code == -8, lens
    ix = sa.ref_index_build(["a"], [L.shared_reference()[2]], device=-1)
    read = L.shared_reference()[2][100:400]
    for prm in (sa.locate_params(read_bases=14), sa.locate_params(read_bases=2049), sa.locate_params(max_occ=0),
                sa.locate_params(max_occ=65537), sa.locate_params(span=0), sa.locate_params(span=8193), sa.locate_params(min_votes=0),
                sa.locate_params(max_hits=512), sa.locate_params(max_hits=16384), sa.locate_params(max_hits=3000)):
        with pytest.raises(sa.SaError) as e:
            sa.guide_locate_batch(ix, [read], prm)
        assert e.value.code == -1
    assert sa.lib().sa_guide_locate_batch(ix._h, None, None, 1, None, 0, (sa._capi.LocateResult * 1)(), None) == -1
    assert sa.lib().sa_guide_locate_batch(ix._h, None, None, -1, None, 0, (sa._capi.LocateResult * 1)(), None) == -1
    with pytest.raises(sa.SaError) as e:                    # a read above 2^24 (the length alone: nothing is read)
        arr, ln = (C.c_char_p * 1)(b"ACGT"), (C.c_int64 * 1)(2 ** 24 + 1)
        sa._capi._chk(sa.lib().sa_guide_locate_batch(ix._h, arr, ln, 1, None, 0, (sa._capi.LocateResult * 1)(), None), "locate")
    assert e.value.code == -1
    # a host-only index has no device to work on, and there is no CPU fallback
    with pytest.raises(sa.SaError) as e:
        sa.guide_locate_batch(ix, [read])
    assert e.value.code == -3


def test_abi_exports_the_locate_symbols():
    Lb = sa.lib()
    names = ("sa_ref_index_build", "sa_ref_index_build_fasta", "sa_ref_index_info", "sa_ref_index_entries", "sa_ref_index_contig",
             "sa_ref_index_destroy", "sa_guide_locate_batch", "sa_locate_release", "sa_locate_window")
    header = open(os.path.join(ROOT, "include", "signalalign_hip.h")).read()
    for name in names:
        assert hasattr(Lb, name) and name in header and name in sa._capi.EXPORTS, name
    for name in ("sa_ref_index_t", "sa_ref_index_info_t", "sa_locate_params_t", "sa_locate_result_t", "SA_LOCATE_NONE",
                 "SA_LOCATE_AMBIGUOUS", "SA_LOCATE_OVERFLOW", "SA_LOCATE_EMPTY"):
        assert name in header, name
    p = sa.locate_params()
    assert (p.read_bases, p.max_occ, p.span, p.min_votes, p.max_hits) == tuple(L.DEFAULTS[f] for f in
                                                                              ("read_bases", "max_occ", "span", "min_votes", "max_hits"))
    assert (sa.LOCATE_NONE, sa.LOCATE_AMBIGUOUS, sa.LOCATE_OVERFLOW, sa.LOCATE_EMPTY) == (L.NONE, L.AMBIGUOUS, L.OVERFLOW, L.EMPTY)
    assert sa.LOCATE_FIELDS == L.FIELDS


def _cli(*args):
    model = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
    return subprocess.run([BIN, "-T", model] + list(args), capture_output=True, text=True, timeout=60)


def test_guide_locate_is_refused_next_to_a_cigar_a_window_and_rna(tmp_path):
    """the refusals need no device"""
    npread = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    pr = _cli("-f", "none.fa", "-q", npread, "--guide-locate", "-p", "x.cigar")
    assert pr.returncode != 0 and "--guide-locate excludes -p and --guide-window" in pr.stderr
    pr = _cli("-f", "none.fa", "-q", npread, "--guide-locate", "--guide-window", "chrE:1-2")
    assert pr.returncode != 0 and "--guide-locate excludes -p and --guide-window" in pr.stderr
    pr = _cli("-f", "none.fa", "-q", npread, "--guide-locate", "--rna")
    assert pr.returncode != 0 and "cannot be combined with --rna" in pr.stderr
    pr = _cli("-q", npread, "--guide-locate")
    assert pr.returncode != 0 and "--guide-locate needs -f <fasta>" in pr.stderr
    manifest = str(tmp_path / "m.tsv")
    with open(manifest, "w") as f:
        f.write("r1\t%s\t@\t%s\n" % (npread, str(tmp_path / "o.tsv")))
    pr = _cli("-f", "none.fa", "--rna", "--batch", manifest)
    assert pr.returncode != 0 and "cannot be combined with --rna" in pr.stderr
    assert not os.path.exists(str(tmp_path / "o.tsv"))
