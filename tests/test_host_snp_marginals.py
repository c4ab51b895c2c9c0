"""CPU checks of the host side of the marginals over reads (sa_snp_marginals_*, sa_snp_group_sites, sa_snp_substitute_sites,
sa_snp_apply_calls, sa_snp_write_marginals): header, export list and ctypes agree on the new names, the helpers equal the
restatement in snp_marginals_ref.py, and without a GPU the accumulator refuses."""
import random
import re

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi

from abi_header import header_text

import snp_marginals_ref as ref

NEW = ["sa_snp_marginals_create", "sa_snp_marginals_destroy", "sa_snp_marginals_add_sites", "sa_snp_marginals_add_batch",
       "sa_snp_marginals_checkpoint", "sa_snp_marginals_rollback", "sa_snp_marginals_finish", "sa_snp_group_sites",
       "sa_snp_substitute_sites", "sa_snp_apply_calls", "sa_snp_write_marginals"]


def test_header_exports_and_ctypes_agree():
    hdr = header_text()
    declared = set(re.findall(r"\b(sa_snp_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared
    assert declared <= set(_capi.EXPORTS)
    L = sa.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
        # one ctypes argument per parameter of the declaration
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(fn.argtypes) == len(decl.split(",")), name
    # the structures the calls exchange have the header's sizes
    assert _capi.SNP_MARGINAL_DTYPE.itemsize == 128 and _capi.SNP_SITE_DTYPE.itemsize == 48
    import ctypes as C
    assert C.sizeof(_capi.SnpJobMap) == 56


def _chain(start, gap, n):
    return [start + gap * i for i in range(n)]


GROUP_CASES = {
    "none": [],
    "one": [(40, 0.3)],
    "two close": [(40, 0.3), (43, 0.5)],
    "two apart": [(40, 0.3), (60, 0.5)],
    "chain of 5 apart": [(p, d) for p, d in zip(_chain(100, 5, 7), [0.1, 0.4, 0.2, 0.9, 0.3, 0.9, 0.05])],
    "gaps of exactly 6": [(p, 0.2 + 0.01 * i) for i, p in enumerate(_chain(10, 6, 5))],
    "equal deltas": [(10, 0.5), (12, 0.5), (14, 0.5), (30, 0.25), (31, 0.25)],
    "trailing lone site": [(10, 0.1), (12, 0.6), (50, 0.2), (52, 0.1), (90, 0.7)],
    "unsorted": [(52, 0.1), (10, 0.1), (90, 0.7), (12, 0.6), (50, 0.2), (91, 0.8), (13, 0.6)],
}


@pytest.mark.parametrize("keep_last", [False, True])
@pytest.mark.parametrize("name", sorted(GROUP_CASES))
def test_group_sites(name, keep_last):
    sites = GROUP_CASES[name]
    got = sa.snp_group_sites([s[0] for s in sites], [s[1] for s in sites], 6, keep_last)
    assert got == ref.group_sites(sites, 6, keep_last), name


def test_group_sites_known_answers():
    # written out by hand from group_sites_in_window: the trailing lone site is lost unless keep_last
    t = GROUP_CASES["trailing lone site"]
    assert sa.snp_group_sites([s[0] for s in t], [s[1] for s in t], 6, False) == [12, 50]
    assert sa.snp_group_sites([s[0] for s in t], [s[1] for s in t], 6, True) == [12, 50, 90]
    assert sa.snp_group_sites([40], [0.3], 6, False) == [] and sa.snp_group_sites([40], [0.3], 6, True) == [40]
    c = GROUP_CASES["chain of 5 apart"]
    assert sa.snp_group_sites([s[0] for s in c], [s[1] for s in c], 6, True) == [115]      # one group, the first 0.9
    g = GROUP_CASES["gaps of exactly 6"]
    assert sa.snp_group_sites([s[0] for s in g], [s[1] for s in g], 6, True) == [10, 16, 22, 28, 34]
    assert sa.snp_group_sites([s[0] for s in g], [s[1] for s in g], 6, False) == [10, 16, 22, 28]
    e = GROUP_CASES["equal deltas"]
    assert sa.snp_group_sites([s[0] for s in e], [s[1] for s in e], 6, True) == [10, 30]
    rng = random.Random(5)
    for _ in range(200):
        sites = [(rng.randrange(0, 300), rng.choice([0.1, 0.2, 0.2, 0.7, rng.random()])) for _ in range(rng.randrange(0, 40))]
        for keep in (False, True):
            assert sa.snp_group_sites([s[0] for s in sites], [s[1] for s in sites], 6, keep) == ref.group_sites(sites, 6, keep)


def _revcomp(s):
    pair = {"A": "T", "C": "G", "G": "C", "T": "A"}
    return "".join(pair.get(c, c) for c in reversed(s))


@pytest.mark.parametrize("step", [1, 3, 5, 10])
def test_substitute_sites_equals_the_periodic_substitution(step):
    rng = random.Random(step)
    record = "".join(rng.choice("ACGTacgt") for _ in range(400))
    for phase in range(step):
        sites = list(range(phase, 400, step))   # the whole contig's sites: most lie outside a window
        for lo, hi in ((0, 399), (17, 250), (133, 134), (391, 399)):
            window = record[lo:hi + 1]
            assert sa.snp_substitute_sites(window, lo, sites) == sa.snp_substitute(window, lo, False, step, phase)
            target = _revcomp(window.upper()).lower() if phase % 2 else _revcomp(window.upper())
            assert sa.snp_substitute_sites(target, hi, sites, reversed=True) == sa.snp_substitute(target, hi, True, step, phase)
    assert sa.snp_substitute_sites("acgtac", 100, [0, 99, 101, 106, 5000]) == "AXGTAC"
    assert sa.snp_substitute_sites("acgtac", 105, [0, 99, 101, 106, 5000], reversed=True) == "ACGTXC"
    assert sa.snp_substitute_sites("acgt", 7, []) == "ACGT"
    with pytest.raises(sa.SaError):
        sa.snp_substitute_sites("ACGT", 0, [3, 1])   # not ascending


def _sites():
    rows = [
        # (contig, pos, run, strand, direction, p)
        (0, 3, 0, 0, 1, (0.7, 0.1, 0.1, 0.1)), (0, 3, 1, 0, 0, (0.05, 0.05, 0.1, 0.8)), (0, 9, 0, 0, 1, (0.1, 0.2, 0.30000000000000004, 0.4)),
        (0, 11, 1, 0, 1, (0.0, 0.0, 0.0, 0.0)), (1, 0, 2, 0, 1, (1e-07, 0.5, 0.25, 0.25)), (1, 6, 2, 1, 0, (0.25, 0.25, 0.25, 0.25)),
    ]
    refs = ["ACGTACGTACGTAC", "ggggggn"]
    return ref.finish(ref.accumulate([rows]), 1, refs), refs


def _as_array(sites):
    arr = np.zeros(len(sites), dtype=_capi.SNP_MARGINAL_DTYPE)
    for a, s in zip(arr, sites):
        a["pos"], a["contig"], a["depth"], a["delta"] = s["pos"], s["contig"], s["depth"], s["delta"]
        a["fwd"], a["bwd"], a["prob"] = s["fwd"], s["bwd"], s["prob"]
        a["called"], a["ref"], a["is_proposal"] = s["called"].encode(), s["ref"].encode(), int(s["is_proposal"])
    return arr


def test_apply_calls_and_write_marginals(tmp_path):
    sites, refs = _sites()
    assert [s["is_proposal"] for s in sites] == [True, True, False, True, False]   # T -> A; C -> T; total 0; g -> C; n
    arr = _as_array(sites)
    for contig, r in enumerate(refs):
        assert sa.snp_apply_calls(r, arr, contig) == ref.apply_calls(r, sites, contig)
    assert sa.snp_apply_calls(refs[0], arr, 0) == "ACGAACGTATGTAC" and sa.snp_apply_calls(refs[1], arr, 1) == "Cgggggn"
    path = str(tmp_path / "m.tsv")
    sa.snp_write_marginals(path, ["chr_a", "chr_b"], arr)
    text = open(path).read()
    assert text == ref.marginals_file(sites, ["chr_a", "chr_b"])
    lines = text.splitlines()
    assert lines[2] == "chr_a\t11\t1\t0.0\t0.0\t0.0\t0.0\tN\tT\t0.0"
    assert lines[4] == "chr_b\t6\t1\t0.25\t0.25\t0.25\t0.25\tA\tN\t0.0"
    sa.snp_write_marginals(path, ["chr_a", "chr_b"], arr[:0])
    assert open(path).read() == ""


def test_no_device_fails_loudly():
    if sa.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(sa.SaError) as ei:
        sa.SnpMarginals([1000, 500], step=5)
    assert ei.value.code == -3
