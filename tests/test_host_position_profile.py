"""CPU checks of the host side of the per-position profile (sa_position_profile_*, sa_profile_entropy_term): header, export list and
ctypes agree on the new names, the entropy term equals the formula, the writer equals the restatement in profile_ref.py byte for
byte, the restatement gives a hand-computed answer, and without a GPU the accumulator refuses."""
import ctypes as C
import re

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi

from abi_header import header_text

import profile_ref as ref

NEW = ["sa_position_profile_create", "sa_position_profile_destroy", "sa_position_profile_add_batch", "sa_position_profile_add_records",
       "sa_position_profile_checkpoint", "sa_position_profile_rollback", "sa_position_profile_finish", "sa_position_profile_write",
       "sa_profile_entropy_term"]


def test_header_exports_and_ctypes_agree():
    hdr = header_text()
    declared = set(re.findall(r"\b(sa_(?:position_)?profile_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) == declared
    assert declared <= set(_capi.EXPORTS)
    L = sa.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
        # one ctypes argument per parameter of the declaration
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(fn.argtypes) == len(decl.split(",")), name
    # the structures the calls exchange have the header's sizes
    assert _capi.PROFILE_SITE_DTYPE.itemsize == 176 and C.sizeof(_capi.ProfileJobMap) == 16
    assert sa.PROFILE_DIRECT == int(re.search(r"#define SA_PROFILE_DIRECT (\d+)u", hdr).group(1))


def test_entropy_term_against_the_formula():
    L = sa.lib()
    got = np.array([L.sa_profile_entropy_term(u) for u in range(ref.UNITS_1 + 1)], dtype=np.int64)
    want = np.array([ref.entropy_term(u) for u in range(ref.UNITS_1 + 1)], dtype=np.int64)
    assert got[0] == 0 and got[ref.UNITS_1] == 0
    assert got[500000] == -2 ** 40
    assert np.array_equal(got, got[::-1])                # u <-> 10^6 - u
    # two log2 implementations, each far more exact than 2^-40: they can only differ across a rounding boundary
    assert np.abs(got - want).max() <= 1
    assert (got[1:ref.UNITS_1] < 0).all() and got.min() == -2 ** 40
    assert L.sa_profile_entropy_term(-1) == 0 and L.sa_profile_entropy_term(ref.UNITS_1 + 1) == 0


def _as_array(sites):
    arr = np.zeros(len(sites), dtype=_capi.PROFILE_SITE_DTYPE)
    for a, s in zip(arr, sites):
        for f in ("pos", "contig", "read_count", "kmer_count", "entropy_units", "entropy"):
            a[f] = s[f]
        a["units"][:len(s["units"])] = s["units"]
        a["prob"][:len(s["prob"])] = s["prob"]
        a["ref"] = s["ref"].encode()
    return arr


def test_known_answer_of_the_restatement():
    # k = 5.  A forward file: ACGTA at 10 printed 0.500000, CGTAC at 11 printed 0.250000: letters at 10..14 and 11..15.
    # A backward file: AACCG at 14 printed 1.000000: letter i lies at 14 - i + 4 and is complemented: T 18, T 17, G 16, G 15, C 14.
    fwd = "c\t10\tACGTA\tr\tt\t0\t0\t0\t0\tACGTA\t0\t0\t0.500000\t0\t0\tACGTA\nc\t11\tCGTAC\tr\tt\t1\t0\t0\t0\tCGTAC\t0\t0\t0.250000\t0\t0\tCGTAC\n"
    bwd = "c\t14\tCGGTT\tq\tt\t0\t0\t0\t0\tAACCG\t0\t0\t1.000000\t0\t0\tAACCG\n"
    assert ref.is_forward_alignment(fwd) is True and ref.is_forward_alignment(bwd) is False
    P = ref.Profile()
    P.add_file(ref.rows_of_tsv(fwd), True)
    P.add_file(ref.rows_of_tsv(bwd), False)
    sites = P.finish("ACGT", ["c"], ["acgtacgtacACGTACGGTnn"])
    half, quarter = -2 ** 40, -892009731203      # the terms of 0.5 and of 0.25; 1.0 has term 0
    assert ref.entropy_term(500000) == half and ref.entropy_term(250000) == quarter and ref.entropy_term(1000000) == 0
    want = [
        # pos, read_count, kmer_count, entropy_units, units (A, C, G, T), prob, entropy, ref
        (10, 1, 1, half, [500000, 0, 0, 0], [1.0, 0.0, 0.0, 0.0], 0.5, "A"),
        (11, 1, 2, half + quarter, [0, 750000, 0, 0], [0.0, 1.0, 0.0, 0.0], 0.4528195311147556, "C"),
        (12, 1, 2, half + quarter, [0, 0, 750000, 0], [0.0, 0.0, 1.0, 0.0], 0.4528195311147556, "G"),
        (13, 1, 2, half + quarter, [0, 0, 0, 750000], [0.0, 0.0, 0.0, 1.0], 0.4528195311147556, "T"),
        (14, 2, 3, half + quarter, [750000, 1000000, 0, 0], [0.42857142857142855, 0.5714285714285714, 0.0, 0.0], 0.30187968740983706, "A"),
        (15, 2, 2, quarter, [0, 250000, 1000000, 0], [0.0, 0.2, 0.8, 0.0], 0.2028195311147556, "C"),
        (16, 1, 1, 0, [0, 0, 1000000, 0], [0.0, 0.0, 1.0, 0.0], 0.0, "G"),
        (17, 1, 1, 0, [0, 0, 0, 1000000], [0.0, 0.0, 0.0, 1.0], 0.0, "G"),
        (18, 1, 1, 0, [0, 0, 0, 1000000], [0.0, 0.0, 0.0, 1.0], 0.0, "T"),
    ]
    assert len(sites) == len(want)
    for s, w in zip(sites, want):
        assert (s["pos"], s["read_count"], s["kmer_count"], s["entropy_units"], s["units"], s["prob"], s["entropy"], s["ref"]) == w
        assert s["contig"] == 0
    assert P.letters_seen("ACGT") == 0b1111
    # rows_of_records is the same rows from job coordinates: the forward job's ref starts at 8, the backward job's index 0 is 20
    Q = ref.Profile()
    Q.add_file(ref.rows_of_records("c", 8, 1, 5, "ACGT", [2, 3], [sa_id("ACGTA"), sa_id("CGTAC")], [5000000, 2500000]), True)
    Q.add_file(ref.rows_of_records("c", 20, -1, 5, "ACGT", [2], [sa_id("AACCG")], [10000000]), False)
    assert Q.finish("ACGT", ["c"], ["acgtacgtacACGTACGGTnn"]) == sites


def sa_id(kmer, alphabet="ACGT"):
    v = 0
    for c in kmer:
        v = v * len(alphabet) + alphabet.index(c)
    return v


def test_write_equals_the_restatement(tmp_path):
    # hand-built: an uncovered-but-spanned position, a letter never seen (G), a zero total, two contigs
    sites = [
        {"contig": 0, "pos": 3, "read_count": 2, "kmer_count": 3, "entropy_units": -2 ** 40 - 892009731203,
         "units": [750000, 1000000, 0, 0, 0], "prob": [0.42857142857142855, 0.5714285714285714, 0.0, 0.0, 0.0],
         "entropy": 0.30187968740983706, "ref": "A"},
        {"contig": 0, "pos": 4, "read_count": 1, "kmer_count": 0, "entropy_units": 0, "units": [0] * 5, "prob": [0.0] * 5, "entropy": 0.0,
         "ref": ""},
        {"contig": 0, "pos": 5, "read_count": 1, "kmer_count": 2, "entropy_units": 0, "units": [0] * 5, "prob": [0.0] * 5, "entropy": 0.0,
         "ref": "N"},
        {"contig": 1, "pos": 0, "read_count": 0, "kmer_count": 7, "entropy_units": -123456789012345,
         "units": [1, 0, 2, 0, 3], "prob": [1 / 6, 0.0, 2 / 6, 0.0, 3 / 6], "entropy": (-123456789012345 * 2.0 ** -40 / 7) / -2.0, "ref": "T"},
        {"contig": 1, "pos": 1099511627775, "read_count": 2147483647, "kmer_count": 2 ** 40, "entropy_units": -1,
         "units": [0, 0, 0, 0, 10 ** 15], "prob": [0.0, 0.0, 0.0, 0.0, 1.0], "entropy": (-1 * 2.0 ** -40 / 2 ** 40) / -2.0, "ref": "E"},
    ]
    alphabet, seen = "ACEGT", 0b10111          # G (bit 3) never seen
    path = str(tmp_path / "p.tsv")
    sa.position_profile_write(path, alphabet, seen, ["chr_a", "chr_b"], _as_array(sites))
    text = open(path).read()
    assert text == ref.file_text(sites, alphabet, seen, ["chr_a", "chr_b"])
    lines = text.splitlines()
    assert lines[0] == ref.HEADER + "\tpA\tpC\tpE\tpT"
    assert lines[2] == "chr_a\t4\t\t0.0\t0\t1\t0.0\t0.0\t0.0\t0.0"
    assert lines[3] == "chr_a\t5\tN\t0.0\t2\t1\t0.0\t0.0\t0.0\t0.0"
    sa.position_profile_write(path, alphabet, 0, ["chr_a", "chr_b"], _as_array(sites)[:0])
    assert open(path).read() == ref.HEADER + "\n"
    with pytest.raises(sa.SaError):
        sa.position_profile_write(path, "ACGT", 0b10000, ["chr_a"], _as_array(sites)[:0])   # a letter outside the alphabet


def test_create_refuses_alphabets_it_cannot_hold():
    # checked before the device is looked at: a letter whose complement is missing, more letters than a site holds
    for alphabet in ("ACG", "ABCDEFGHI"):
        n = len(alphabet) ** 2
        m = sa.Model.create(alphabet, 2, np.full(10, 0.1), np.tile([60.0, 1.0, 1.0, 0.1, 1.0], n))
        with pytest.raises(sa.SaError) as ei:
            sa.PositionProfile(m, [100])
        assert ei.value.code == -8, alphabet


def test_no_device_fails_loudly():
    if sa.device_count() > 0:
        pytest.skip("a GPU is present")
    from sa_cases import MODEL_R73
    m = sa.Model.load(MODEL_R73)
    with pytest.raises(sa.SaError) as ei:
        sa.PositionProfile(m, [1000, 500])
    assert ei.value.code == -3
