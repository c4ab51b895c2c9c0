"""CPU checks around the k-mer mixture fit: the numpy restatement (kmer_mixture_ref.py) against sklearn, live and as recorded
in tests/golden/mixture/, the two host helpers against the restatement and the reference's recorded pairs, and the ABI."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi

import kmer_mixture_ref as ref
import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = os.path.join(cases.GOLDEN, "mixture")
# the restatement and sklearn do the same arithmetic in another order of operations: 1e-11 is ten times the worst difference
# seen over random cases (9.1e-13), relative to max(1, |value|)
BAR = 1e-11


def _compare(name, got, w, m, s, n_iter, conv, lb):
    worst = max(np.abs(got["weight"] - w).max(), (np.abs(got["mean"] - m) / np.maximum(1.0, np.abs(m))).max(),
                (np.abs(got["sd"] - s) / np.maximum(1.0, s)).max(), abs(got["lower_bound"] - lb) / max(1.0, abs(lb)))
    assert worst <= BAR, (name, worst)   # (a NaN fails this too)
    assert (got["n_iter"], got["converged"]) == (n_iter, conv), name
    return worst


def _near_threshold(changes, tol, rel=1e-3):
    return tol > 0 and any(abs(c - tol) <= rel * tol for c in changes)


def test_restatement_matches_live_sklearn():
    pytest.importorskip("sklearn")
    worst = 0.0
    for name, x, K, max_iter, tol in ref.host_cases():
        changes = []
        got = ref.fit(x, K, max_iter=max_iter, tol=tol, changes=changes)
        assert not _near_threshold(changes, tol), name   # (an iteration count could then differ for rounding alone)
        worst = max(worst, _compare(name, got, *ref.sklearn_fit(x, K, max_iter, tol)))
    print("restatement vs sklearn: worst difference %.3g" % worst)


def test_restatement_matches_recorded_sklearn():
    z = np.load(os.path.join(MIX, "sklearn_fits.npz"))
    for name, x, K, max_iter, tol in ref.host_cases():
        got = ref.fit(x, K, max_iter=max_iter, tol=tol)
        n_iter, conv = (int(v) for v in z[name + "_iter"])
        _compare(name, got, z[name + "_weight"], z[name + "_mean"], z[name + "_sd"], n_iter, conv, float(z[name + "_lb"][0]))


def test_fixed_iteration_cases_run_every_iteration():
    x = ref.planted(7, 300, ref.TWO)
    got = ref.fit(x, 2, max_iter=25, tol=0.0)
    assert got["n_iter"] == 25 and got["converged"] == 0
    assert ref.fit(x[:1], 2)["status"] == 1


def test_motif_kmer_pairs_match_the_reference():
    recorded = json.load(open(os.path.join(MIX, "motif_pairs.json")))
    seen = set()
    for c in recorded:
        exp = [tuple(p) for p in c["pairs"]]
        got = sa.motif_kmer_pairs(c["k"], c["canonical"], c["modified"], c["alphabet"])
        assert got == exp, (c["k"], c["canonical"], c["alphabet"])
        assert got == ref.motif_kmer_pairs(c["k"], c["canonical"], c["modified"], c["alphabet"])
        assert got == sorted(set(got)) and all(len(a) == c["k"] == len(b) for a, b in got)
        seen.add((c["k"], c["canonical"], len(c["canonical"]) > c["k"]))
    for k in (5, 6):
        assert (k, "CCAGG", False) in seen and (k, "CCTGG", False) in seen
    assert any(longer for _, _, longer in seen)
    # the default alphabet is the reference's "ATGC"
    assert sa.motif_kmer_pairs(6, "CCAGG", "CEAGG") == sa.motif_kmer_pairs(6, "ccagg", "ceagg", "ATGC")


def test_motif_kmer_pairs_first_occurrence_quirk():
    # a flank that carries the new letter: only its FIRST occurrence becomes the old letter
    got = sa.motif_kmer_pairs(4, "AC", "EC", "ACE")
    assert ("AEEC", "EEEC") in got and ("AAEC", "EAEC") in got and ("AAEC", "AAEC") not in got


def test_motif_kmer_pairs_errors():
    for args in ((6, "CCAGG", "CEAG"), (6, "CCAGG", "CCAGG"), (6, "CCAGG", "CEEGG"), (6, "CXAGG", "CEAGG"), (0, "CCAGG", "CEAGG"),
                 (17, "CCAGG", "CEAGG")):
        with pytest.raises(sa.SaError) as ei:
            sa.motif_kmer_pairs(*args)
        assert ei.value.code == -1, args


def _fit(means, status=0):
    f = np.zeros(1, dtype=sa.MIXTURE_FIT_DTYPE)
    f["mean"][0, :2] = means
    f["status"] = status
    return f


def test_mixture_assign():
    assert sa.mixture_assign(_fit([78.0, 84.0]), 83.0) == (1, 0, 1.0)
    assert sa.mixture_assign(_fit([78.0, 84.0]), 79.0) == (0, 1, 1.0)
    # a tie: the first minimal index (strict <)
    assert sa.mixture_assign(_fit([80.0, 84.0]), 82.0) == (0, 1, 2.0)
    assert sa.mixture_assign(_fit([84.0, 80.0]), 82.0) == (0, 1, 2.0)
    # nothing nearer than 1000: component 0 and the initial distance; exactly 1000 is not nearer
    assert sa.mixture_assign(_fit([5000.0, 2000.0]), 0.0) == (0, 1, 1000.0)
    assert sa.mixture_assign(_fit([1000.0, 3000.0]), 0.0) == (0, 1, 1000.0)
    assert sa.mixture_assign(_fit([1500.0, 999.5]), 0.0) == (1, 0, 999.5)
    for means, c in (([78.0, 84.0], 83.0), ([80.0, 84.0], 82.0), ([5000.0, 2000.0], 0.0), ([1500.0, 999.5], 0.0)):
        assert sa.mixture_assign(_fit(means), c) == ref.assign(means, c)
    with pytest.raises(sa.SaError) as ei:
        sa.mixture_assign(_fit([78.0, 84.0], status=1), 80.0)
    assert ei.value.code == -1


def test_header_exports_and_ctypes_agree():
    hdr = open(os.path.join(ROOT, "include", "signalalign_hip.h")).read()
    L = sa.lib()
    for name in ("sa_kmer_table_mixture", "sa_kmer_table_mixture_start", "sa_mixture_assign", "sa_motif_kmer_pairs"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _capi.EXPORTS and hasattr(L, name), name
    # struct layouts: the header's fields in order, the ctypes / numpy mirrors of the same size and offsets
    body = re.search(r"typedef struct sa_mixture_fit \{(.*?)\} sa_mixture_fit_t;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip()
              for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == list(sa.MIXTURE_FIT_DTYPE.names)
    assert sa.MIXTURE_FIT_DTYPE.itemsize == 128 and sa.MIXTURE_FIT_DTYPE.fields["lower_bound"][1] == 24
    assert re.search(r"typedef struct sa_mixture_params \{ int32_t n_components, max_iter; double tol, reg_covar; \}", hdr)
    assert [f[0] for f in sa.MixtureParams._fields_] == ["n_components", "max_iter", "tol", "reg_covar"]
    assert C.sizeof(sa.MixtureParams) == 24
