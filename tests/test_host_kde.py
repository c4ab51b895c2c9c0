"""CPU checks around the two comparisons of a model with its data (sa_kmer_table_kde, sa_hdp_state_vs_gaussian): the ABI, the
restatements of tests/kde_ref.py against what scikit-learn and scipy gave (tests/golden/kde/, written by
tests/golden/make_kde_fixtures.py), and the argument checks that come before any device use.

Bars of the restatement against the libraries, relative to max(1, |value|): 1e-13.  Both sides do the same arithmetic in
another order; an exponent is rounded a handful of times on either side (a few 1e-16 of a value it dominates) and a sum over
at most 76 rows or 100 grid points moves by at most that many half-ulps (8e-15): the bar is ten times the sum of the two."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi, synth

import kde_ref as ref
import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDE = os.path.join(cases.GOLDEN, "kde")
ASSIGNMENTS = os.path.join(cases.GOLDEN, "hdp", "d6160b0b-a35e-43b5-947f-adaa1abade28.sm.assignments.tsv.gz")
BAR = 1e-13


def rel(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    return float((np.abs(got - exp) / np.maximum(1.0, np.abs(exp))).max())


def test_header_exports_and_ctypes_agree():
    hdr = open(os.path.join(ROOT, "include", "signalalign_hip.h")).read()
    L = sa.lib()
    for name in ("sa_kmer_table_kde", "sa_hdp_state_vs_gaussian"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _capi.EXPORTS and hasattr(L, name), name
    assert re.search(r"typedef struct sa_hdp_gauss_cmp \{ double kl_bits, hellinger, mode_delta; int32_t status, pad; \} "
                     r"sa_hdp_gauss_cmp_t;", hdr)
    assert list(sa.HDP_GAUSS_CMP_DTYPE.names) == ["kl_bits", "hellinger", "mode_delta", "status", "pad"]
    assert sa.HDP_GAUSS_CMP_DTYPE.itemsize == 32 and sa.HDP_GAUSS_CMP_DTYPE.fields["status"][1] == 24
    assert hasattr(sa.KmerTable, "kde") and hasattr(sa.HdpState, "vs_gaussian")
    # the reference's lines both blocks restate
    assert "hiddenMarkovModel.py:654-773" in hdr and "hiddenMarkovModel.py:775-837" in hdr and ":1119-1120" in hdr


def test_kde_restatement_reproduces_sklearn():
    z = np.load(os.path.join(KDE, "sklearn_kde.npz"))
    per = {}
    with gzip.open(ASSIGNMENTS, "rt") as f:
        for ln in f:
            t = ln.split()
            if t:
                per.setdefault(t[0], []).append(float(t[2]))
    kmers, n_rows = [str(k) for k in z["kmers"]], z["n_rows"]
    assert len(kmers) == 64 and (n_rows == 1).sum() == 4 and n_rows.max() > 50
    assert np.array_equal(z["x"], np.linspace(30.0, 90.0, 600)) and float(z["bandwidth"][0]) == 0.5
    worst = 0.0
    for i, k in enumerate(kmers):
        assert len(per[k]) == n_rows[i]
        units = [sa.f6_units(v)[0] for v in per[k]]
        got = ref.kde_log_density(units, z["x"], 0.5)
        assert np.isfinite(got).all()
        worst = max(worst, rel(got, z["log_density"][i]))
    print("KDE restatement vs sklearn: worst difference %.3g, lowest log density %.1f" % (worst, z["log_density"].min()))
    assert worst <= BAR
    assert z["log_density"].min() < -5000   # (the fixture reaches far below what exp can hold without the shift)


def test_kde_cut_and_order_properties():
    rng = np.random.RandomState(3)
    units = np.round(rng.normal(80.0, 2.0, 300) * 1e6).astype(np.int64)
    x = np.linspace(30.0, 90.0, 97)
    a = ref.kde_log_density(units, x, 0.5)
    # against scipy's logsumexp over every row (no cut): the cut leaves out less than n exp(-64)
    pytest.importorskip("scipy")
    assert rel(a, ref.kde_closed_form(units, x, 0.5)) <= BAR
    # the order of the input does not matter (the rows are sorted first); one row: the kernel itself
    assert np.array_equal(a, ref.kde_log_density(units[::-1], x, 0.5))
    one = ref.kde_log_density([75000000], [75.0, 76.0], 0.5)
    assert one[0] == -(np.log(0.5) + ref.HALF_LOG_2PI) and abs(one[1] - (one[0] - 2.0)) <= 1e-15
    assert np.all(np.isneginf(ref.kde_log_density([], x, 0.5)))


@pytest.fixture(scope="module")
def hdp():
    s = sa.HdpState(cases.NHDP)
    yield s
    s.close()


def test_hdp_vs_gaussian_restatement_reproduces_scipy(hdp):
    z = np.load(os.path.join(KDE, "scipy_hdp_vs_gaussian.npz"))
    alpha, k, _, tab = synth.parse_model_table(cases.MODEL_R73)
    tab = np.asarray(tab).reshape(-1, 5)
    observed, row_of, post, grid = hdp.array("observed"), hdp.array("row_of_dp"), hdp.array("post"), hdp.array("grid")
    ids = z["dp_ids"]
    assert len(ids) == 351 and np.array_equal(ids, np.flatnonzero(observed[:len(alpha) ** k]))
    assert np.array_equal(z["mean"], tab[ids, 0]) and np.array_equal(z["sd"], tab[ids, 1])
    assert list(z["sd_scales"]) == [1.0, 4.0]
    finite = {}
    for scale in (1, 4):
        kl, hel, delta = (z["%s_x%d" % (n, scale)] for n in ("kl_bits", "hellinger", "mode_delta"))
        finite[scale] = int(np.isfinite(kl).sum())
        assert not np.isnan(kl).any()
        worst = 0.0
        for j, dp in enumerate(ids):
            g_kl, g_hel, g_delta, status = ref.hdp_vs_gaussian(post[row_of[dp]], grid, z["mean"][j], scale * z["sd"][j])
            assert status == (0 if np.isfinite(kl[j]) else 2), (scale, dp)
            if status == 0:
                worst = max(worst, rel(g_kl, kl[j]))
            else:
                assert g_kl == kl[j] == np.inf
            worst = max(worst, rel(g_hel, hel[j]))
            assert g_delta == delta[j]
        print("HDP vs Gaussian restatement vs scipy at %d x sd: worst difference %.3g" % (scale, worst))
        assert worst <= BAR
    assert finite == {1: 12, 4: 351}   # both status paths, defined by scipy alone


def test_rel_entr_branches():
    pytest.importorskip("scipy")
    from scipy.special import rel_entr
    for a, b in ((0.3, 0.4), (0.3, 1e-5), (1e-5, 0.3), (0.3, 5e-324), (0.3, 1e-310), (1e-310, 0.3), (0.0, 0.0), (0.0, 0.2), (0.2, 0.0),
                 (1e-300, 1e300), (1e300, 1e-300)):
        e, g = float(rel_entr(a, b)), ref.rel_entr(a, b)
        assert g == e or abs(g - e) <= 4e-16 * abs(e), (a, b, g, e)
    # the naive a log(a / b) is not finite where the quotient overflows
    assert np.isfinite(ref.rel_entr(0.3, 5e-324)) and np.isinf(0.3 / 5e-324)


def test_vs_gaussian_argument_checks_come_before_the_device(hdp):
    L = sa.lib()
    out = np.zeros(4, dtype=sa.HDP_GAUSS_CMP_DTYPE)
    ip, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)

    def call(ids, mean, sd, state=None, null=None):
        i, m, s = np.asarray(ids, dtype=np.int64), np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
        args = [hdp._h if state is None else state, i.ctypes.data_as(ip), len(i), m.ctypes.data_as(dp), s.ctypes.data_as(dp), 0,
                out.ctypes.data, None]
        if null is not None:
            args[null] = None
        return L.sa_hdp_state_vs_gaussian(*args)

    EINVAL, ESTATE = -1, call([0], [50.0], [1.0], state=_unfinalised()._h)
    assert sa.lib().sa_strerror(EINVAL) and ESTATE not in (0, EINVAL)
    n_dps = int(hdp.info.num_dps)
    for null in (0, 1, 3, 4, 6):
        assert call([0], [50.0], [1.0], null=null) == EINVAL, null
    assert call([-1], [50.0], [1.0]) == EINVAL and call([n_dps], [50.0], [1.0]) == EINVAL
    for bad in (float("nan"), float("inf")):
        assert call([0], [bad], [1.0]) == EINVAL and call([0], [50.0], [bad]) == EINVAL
    assert call([0], [50.0], [0.0]) == EINVAL and call([0], [50.0], [-1.0]) == EINVAL
    assert L.sa_hdp_state_vs_gaussian(hdp._h, None, -1, None, None, 0, out.ctypes.data, None) == EINVAL
    # a bad argument is reported even for a state that is not finalised, and nothing of this needed a GPU
    assert call([-1], [50.0], [1.0], state=_unfinalised()._h) == EINVAL
    assert call([], [], []) == 0
    if sa.device_count() < 1:
        enodevice = call([0], [50.0], [1.0])
        assert enodevice not in (0, EINVAL, ESTATE)
        with pytest.raises(sa.SaError) as ei:
            hdp.vs_gaussian([0], [50.0], [1.0])
        assert ei.value.code == enodevice


_KEEP = []


def _unfinalised():
    if not _KEEP:
        _KEEP.append(sa.HdpState.new(sa.HDP_LAYOUT_FLAT, "ACGT", 3, (0.0, 100.0, 50), (50.0, 1.0, 2.0, 10.0), gamma=[1.0, 1.0]))
    return _KEEP[0]
