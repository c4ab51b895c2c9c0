"""An HDP's stored distributions against a Gaussian table on the GPU (sa_hdp_state_vs_gaussian) against the plain-Python
restatement (tests/kde_ref.py) and against scipy's own numbers (tests/golden/kde/scipy_hdp_vs_gaussian.npz): every DP of
the bundled .nhdp, both sd scales of the fixture (at the model's sd most normal densities underflow on the 100-point grid and
scipy's entropy is infinite: status 2; at four times that sd all are finite), an id list with repeats and out of order, and
the error contract.

The parity bar is measured in the test: d = max(1e-13, worst difference between the restatement with its sums in grid order
and from the last grid point down), the noise floor of the summation order; the GPU has to be within 100 d (the factor is for
the device's exp / log / sqrt, a few ulp each).  Differences are taken relative to max(1, |value|)."""
import os

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import kde_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

SCIPY = os.path.join(cases.GOLDEN, "kde", "scipy_hdp_vs_gaussian.npz")
FIELDS = ("kl_bits", "hellinger", "mode_delta")


def rel(got, exp):
    return abs(got - exp) / max(1.0, abs(exp))


@pytest.fixture(scope="module")
def hdp():
    s = sa.HdpState(cases.NHDP)
    yield s
    s.close()


@pytest.fixture(scope="module")
def table():
    alpha, k, _, tab = synth.parse_model_table(cases.MODEL_R73)
    return np.asarray(tab).reshape(-1, 5)


@pytest.fixture(scope="module")
def restated(hdp):
    """the fixture's 351 DPs at both sd scales through the restatement, in grid order and reversed (computed once)"""
    z = np.load(SCIPY)
    row_of, post, grid = hdp.array("row_of_dp"), hdp.array("post"), hdp.array("grid")
    fwd, rev = {}, {}
    for scale in (1, 4):
        for j, dp in enumerate(z["dp_ids"]):
            fwd[scale, int(dp)] = ref.hdp_vs_gaussian(post[row_of[dp]], grid, z["mean"][j], scale * z["sd"][j])
            rev[scale, int(dp)] = ref.hdp_vs_gaussian(post[row_of[dp]], grid, z["mean"][j], scale * z["sd"][j], reverse=True)
    d = 1e-13
    for key, e in fwd.items():
        r = rev[key]
        assert r[3] == e[3]
        d = max([d] + [rel(r[f], e[f]) for f in range(3) if np.isfinite(e[f])])
    return z, fwd, d


def test_every_dp_of_the_bundled_hdp(hdp, table):
    n_dps, n_kmers = int(hdp.info.num_dps), len(table)
    assert n_dps == 46657 and n_kmers == 46656
    ids = np.arange(n_dps)
    mean, sd = np.append(table[:, 0], 50.0), np.append(table[:, 1], 2.0)   # (the base DP has no k-mer: any normal)
    stats = {}
    got = hdp.vs_gaussian(ids, mean, 4.0 * sd, stats=stats)
    observed = hdp.array("observed").astype(bool)
    assert observed[:n_kmers].sum() == 351 and observed[n_kmers]
    assert stats["kernel_ms"] > 0 and not got["pad"].any()
    off = got[~observed]
    assert (off["status"] == 1).all() and not off["kl_bits"].any() and not off["hellinger"].any() and not off["mode_delta"].any()
    on = got[observed]
    assert (on["status"] == 0).all() and np.isfinite(on["kl_bits"]).all() and (on["kl_bits"] > 0).all()
    assert ((on["hellinger"] > 0) & np.isfinite(on["hellinger"])).all() and (on["mode_delta"] >= 0).all()


def test_scipy_fixture_at_both_sd_scales(hdp, restated):
    z, fwd, d = restated
    ids = z["dp_ids"]
    worst = 0.0
    n_status = {}
    for scale in (1, 4):
        got = hdp.vs_gaussian(ids, z["mean"], scale * z["sd"])
        for j, dp in enumerate(ids):
            e, g = fwd[scale, int(dp)], got[j]
            lib_vals = [z["%s_x%d" % (f, scale)][j] for f in FIELDS]
            assert int(g["status"]) == e[3] == (0 if np.isfinite(lib_vals[0]) else 2), (scale, dp)
            n_status[scale, e[3]] = n_status.get((scale, e[3]), 0) + 1
            for f, name in enumerate(FIELDS):
                if f == 0 and e[3] == 2:
                    assert g[name] == e[0] == lib_vals[0] == np.inf   # (left in place)
                    continue
                w = rel(float(g[name]), e[f])
                worst = max(worst, w)
                assert w <= 100 * d, (scale, dp, name, w, d)
                # scipy itself is within 1e-13 of the restatement (tests/test_host_kde.py)
                assert rel(float(g[name]), lib_vals[f]) <= 100 * d + 1e-13, (scale, dp, name)
            assert g["mode_delta"] == e[2]
    print("HDP vs Gaussian: d = %.3g (restatement, grid order against reversed), GPU worst difference = %.3g over 2 x %d entries" %
          (d, worst, len(ids)))
    assert n_status == {(1, 0): 12, (1, 2): 339, (4, 0): 351}


def test_repeated_and_unordered_ids(hdp, restated):
    z, fwd, d = restated
    ids, n_kmers = z["dp_ids"], 46656
    unobserved = [i for i in range(100) if i not in set(ids.tolist())][:2]
    pick = [int(ids[7]), unobserved[0], int(ids[300]), int(ids[7]), n_kmers, int(ids[0]), unobserved[1], int(ids[300])]
    where = {int(dp): j for j, dp in enumerate(ids)}
    mean = [z["mean"][where[p]] if p in where else 60.0 for p in pick]
    sd = [4.0 * z["sd"][where[p]] if p in where else 1.5 for p in pick]
    got = hdp.vs_gaussian(pick, mean, sd)
    whole = hdp.vs_gaussian(ids, z["mean"], 4.0 * z["sd"])
    for g, p in zip(got, pick):
        if p in where:
            assert g.tobytes() == whole[where[p]].tobytes(), p   # an entry does not depend on the others of the call
        elif p == n_kmers:
            assert int(g["status"]) in (0, 2) and g["hellinger"] > 0   # the base DP is observed
        else:
            assert int(g["status"]) == 1 and g["kl_bits"] == 0 and g["hellinger"] == 0 and g["mode_delta"] == 0
    assert got[0].tobytes() == got[3].tobytes() and got[2].tobytes() == got[7].tobytes()
    assert len(hdp.vs_gaussian([], [], [])) == 0


def test_error_contract(hdp):
    def refused(ids, mean, sd, state=hdp):
        with pytest.raises(sa.SaError) as ei:
            state.vs_gaussian(ids, mean, sd)
        return ei.value.code

    n_dps = int(hdp.info.num_dps)
    assert refused([-1], [50.0], [1.0]) == -1 and refused([n_dps], [50.0], [1.0]) == -1
    assert refused([0, n_dps], [50.0, 50.0], [1.0, 1.0]) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert refused([0], [bad], [1.0]) == -1
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        assert refused([0], [50.0], [bad]) == -1
    raw = sa.HdpState.new(sa.HDP_LAYOUT_FLAT, "ACGT", 3, (0.0, 100.0, 50), (50.0, 1.0, 2.0, 10.0), gamma=[1.0, 1.0])
    estate = refused([0], [50.0], [1.0], state=raw)
    assert estate not in (0, -1)
    assert refused([-1], [50.0], [1.0], state=raw) == -1   # the argument checks come first
    raw.close()
    with pytest.raises(sa.SaError):
        hdp.vs_gaussian([0, 1], [50.0], [1.0])
