"""HDP distribution distances on the GPU (sa_hdp_distances and its relatives, kernels in signalalign_amd/csrc/sa_hdpdist.hip; the
compareDistributions drop-in) against the numpy restatement of the reference's expressions (tests/hdp_metric_ref.py).

The rules, everywhere: L2 and Hellinger hold only correctly rounded operations (+ - x / sqrt) in the reference's order, so they
must match bit for bit.  KL and Shannon-Jensen also hold two logarithms per grid point, and the device's log is not glibc's: both
are documented within 1 ulp, so per pair |got - want| <= 4 eps S, S the trapezoid sum of the absolute values of the two log terms
(p log(p/q) and q log(q/p); p log(p/m) / 2 and q log(q/m) / 2) -- twice the 2 ulp the two can differ by.  The Shannon-Jensen distance is the
root of its divergence: bound / (2 sqrt(div)) + eps want, exactly 0 where the divergence is 0, and no pair may have a divergence
within 1000 bounds of zero (hdp_metric_ref.check_against)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import hdp_metric_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "signalalign_amd", "bin", "compareDistributions")
HDP_DATA = os.path.join(cases.GOLDEN, "hdp")
METRICS = ((sa.HDP_METRIC_KL, ref.KL), (sa.HDP_METRIC_HELLINGER, ref.HELLINGER), (sa.HDP_METRIC_L2, ref.L2),
           (sa.HDP_METRIC_SHANNON_JENSEN, ref.SHANNON_JENSEN))


def test_metric_constants_are_the_headers():
    assert [m for m, _ in METRICS] == [r for _, r in METRICS] == [0, 1, 2, 3]


# ---- 1. array level ---------------------------------------------------------------------------------------------------------------
def _mixtures(n_rows, grid_length, seed):
    """a grid that is not equidistant, and two-component Gaussian mixtures + 1e-6 on it"""
    rng = np.random.default_rng(seed)
    grid = np.cumsum(rng.uniform(0.2, 1.0, size=grid_length))
    lo, hi = grid[0], grid[-1]
    m1, m2 = rng.uniform(lo, hi, size=(2, n_rows, 1))
    s1, s2 = rng.uniform(0.05, 0.3, size=(2, n_rows, 1)) * (hi - lo + 1.0)
    w = rng.uniform(0.1, 0.9, size=(n_rows, 1))
    gauss = lambda m, s: np.exp(-0.5 * ((grid[None, :] - m) / s) ** 2) / (s * np.sqrt(2.0 * np.pi))
    return grid, w * gauss(m1, s1) + (1.0 - w) * gauss(m2, s2) + 1e-6


SHAPES = [(2, 2), (3, 5), (65, 33), (130, 100)]   # one pair; odd sizes; a tile and a chunk plus one; three rows of tiles, four chunks


@pytest.fixture(scope="module")
def array_cases():
    out = {}
    for n_rows, grid_length in SHAPES:
        grid, rows = _mixtures(n_rows, grid_length, 100 * n_rows + grid_length)
        out[(n_rows, grid_length)] = (grid, rows, {r: ref.all_pairs(grid, rows, r) for _, r in METRICS})
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_all_pairs_against_the_restatement(array_cases, shape):
    grid, rows, want = array_cases[shape]
    n = shape[0]
    for metric, r in METRICS:
        stats = {}
        got = sa.hdp_distances(grid, rows, metric, stats=stats)
        assert got.shape == (n * (n - 1) // 2,) and stats["kernel_ms"] > 0.0
        dist, acc, s = want[r]
        assert not np.isnan(dist).any()
        ref.check_against(r, got, dist, acc, s, label="%dx%d" % shape)


def test_bands_and_the_paired_entry_point_give_the_same_bits(array_cases):
    """The triangle leaves the device in bands of tile rows through two slabs; a slab of the smallest size makes the three tile rows
    of the 130-row case three bands (the third reuses the first one's slab and pinned buffer).  And the paired entry point runs the
    same point functions, one pair per thread: the same bits as the tiled kernel for every metric, the logarithmic ones included."""
    grid, rows, _ = array_cases[(130, 100)]
    i, j = ref.tri_pairs(130)
    for metric, _ in METRICS:
        whole = sa.hdp_distances(grid, rows, metric)
        sa.hdp_distances_release()               # (the scratch kept between calls comes back on the next call)
        os.environ["SA_HDP_DIST_SLAB"] = "1"
        try:
            banded = sa.hdp_distances(grid, rows, metric)
        finally:
            del os.environ["SA_HDP_DIST_SLAB"]
        assert np.array_equal(whole, banded)
        stats = {}
        paired = sa.hdp_distances_paired(grid, rows[i], rows[j], metric, stats=stats)
        assert np.array_equal(whole, paired) and stats["kernel_ms"] > 0.0


# ---- 2. specials ------------------------------------------------------------------------------------------------------------------
def test_ieee_specials_flow_through():
    """No clamping and no special cases: a zero density is a NaN for KL and Shannon-Jensen (0 * log 0), an integral above one a NaN for
    Hellinger, two bit-identical rows give exactly 0 for KL, Shannon-Jensen and L2 and sqrt(1 - integral of p) for Hellinger."""
    grid, rows = _mixtures(4, 7, 5)
    rows[0, 2] = 0.0
    rows[0, 5] = 0.0
    integral_of = lambda y: float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(grid)))
    rows[1] *= 1.3 / integral_of(rows[1])
    rows[2] *= 0.9 / integral_of(rows[2])
    rows[3] = rows[2]
    i, j = ref.tri_pairs(4)
    where = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(i, j))}
    for metric, r in METRICS:
        got = sa.hdp_distances(grid, rows, metric)
        dist, acc, s = ref.all_pairs(grid, rows, r)
        assert np.array_equal(np.isnan(got), np.isnan(dist)), (metric, got, dist)
        assert np.array_equal(got == 0.0, dist == 0.0), (metric, got, dist)
        if r in (ref.KL, ref.SHANNON_JENSEN):
            assert all(np.isnan(got[where[(k, 0)]]) for k in (1, 2, 3)) and got[where[(3, 2)]] == 0.0
            assert not np.isnan(got[where[(2, 1)]])
        if r == ref.L2:
            assert got[where[(3, 2)]] == 0.0 and not np.isnan(got).any()
        if r == ref.HELLINGER:
            # sqrt(p p) = p exactly, so the pair of identical rows integrates p itself
            hell_acc, _ = ref.integral(grid, rows[3:4], rows[2:3], r)
            assert got[where[(3, 2)]] == np.sqrt(1.0 - hell_acc[0]) and 0.25 < got[where[(3, 2)]] < 0.4
        paired = sa.hdp_distances_paired(grid, rows[i], rows[j], metric)
        assert np.array_equal(paired, got, equal_nan=True)
        ref.check_against(r, got, dist, acc, s, label="specials")
    # an integral above one: the Hellinger distance of the 1.3-row against itself is the square root of a negative number
    assert np.isnan(sa.hdp_distances_paired(grid, rows[1:2], rows[1:2], sa.HDP_METRIC_HELLINGER)[0])


# ---- 3. the bundled model ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled():
    s = sa.HdpState(cases.NHDP)
    grid, post = s.array("grid"), s.array("post")
    want = {r: ref.all_pairs(grid, post, r) for _, r in METRICS}
    yield s, grid, post, want
    s.close()


def test_bundled_model_all_pairs(bundled):
    """templateSingleLevelFixed.nhdp: 352 observed DPs x 100 grid points, 61 776 pairs"""
    s, grid, post, want = bundled
    assert post.shape == (352, 100) and post.min() > 0.0
    i, j = ref.tri_pairs(352)
    same = np.all(post[i] == post[j], axis=1)
    assert same.sum() == 2280
    for metric, r in METRICS:
        got = s.distances(metric)
        dist, acc, s_abs = want[r]
        assert got.shape == (61776,) and not np.isnan(got).any() and not np.isnan(dist).any()
        ref.check_against(r, got, dist, acc, s_abs, label="bundled")
        if r != ref.HELLINGER:
            assert np.all(got[same] == 0.0)
        assert np.array_equal(got, sa.hdp_distances(grid, post, metric))
    sj_div = want[ref.SHANNON_JENSEN][1]
    assert sj_div[sj_div > 0].min() > 1e-15            # (6.9e-15 against a largest bound of 4.0e-18: nothing near the excluded window)


def test_bundled_model_distance_pairs(bundled):
    s, grid, post, want = bundled
    observed, parent, rows = s.array("observed"), s.array("dp_parent"), s.array("row_of_dp")
    base = int(s.info.base_dp)
    leaves = np.arange(int(s.info.num_dps))
    leaves = leaves[(leaves != base) & (parent[leaves] == base)]
    no_data = leaves[observed[leaves] == 0][:2]
    with_data = leaves[observed[leaves] == 1][:6]
    assert len(no_data) == 2 and len(with_data) == 6
    base_row = post[rows[base]][None, :]
    for metric, r in METRICS:
        # two k-mers without data stand for the base DP: different ids, one row -- evaluated, not short-cut
        d = s.distance_pairs(metric, no_data[:1], no_data[1:])
        acc, _ = ref.integral(grid, base_row, base_row, r)
        assert d[0] == ref.final(r, acc)[0]
        assert (d[0] == 0.0) if r != ref.HELLINGER else (0.1 < d[0] < 0.11), (metric, d)      # (the base density holds 0.989 on the grid)
        # (i, j) == (j, i), (i, i) == 0.0 without evaluating (Hellinger of a row with itself is not 0)
        a = np.concatenate([with_data, no_data, [base]])
        ii, jj = np.meshgrid(a, a, indexing="ij")
        m = s.distance_pairs(metric, ii.ravel(), jj.ravel()).reshape(len(a), len(a))
        assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0.0)
        # against the memo of the observed DPs
        tri = s.distances(metric)
        ra = np.array([ref.resolve_row(observed, parent, rows, int(d_)) for d_ in a])
        for x_ in range(len(a)):
            for y_ in range(len(a)):
                hi, lo = max(ra[x_], ra[y_]), min(ra[x_], ra[y_])
                if hi != lo:
                    assert m[x_, y_] == tri[(hi - 1) * hi // 2 + lo], (metric, x_, y_)
    with pytest.raises(sa.SaError) as ei:
        s.distance_pairs(sa.HDP_METRIC_KL, [0], [int(s.info.num_dps)])
    assert ei.value.code == -1


def test_bundled_model_densities(bundled):
    """dir_proc_density: the spline between the knots, its linear continuation outside, clamped at zero -- operation for operation, so
    bit for bit (grid_spline_interp holds only + - x / and one truncation)"""
    s, grid, post, _ = bundled
    slope, observed, parent, rows = s.array("slope"), s.array("observed"), s.array("dp_parent"), s.array("row_of_dp")
    rng = np.random.default_rng(11)
    x = np.concatenate([[-500.0, -3.0, grid[0] - 1e-9], grid[[0, 1, 17, 98, 99]], rng.uniform(grid[0], grid[-1], size=300),
                        np.nextafter(grid[[1, 50, 99]], -np.inf), np.nextafter(grid[[0, 50, 98]], np.inf), [grid[-1] + 1e-9, 130.0, 900.0]])
    ids = np.concatenate([[int(s.info.base_dp)], np.flatnonzero(observed)[[0, 7, 100, 350]], rng.integers(0, int(s.info.num_dps), size=30)])
    got = s.densities(ids, x)
    assert got.shape == (len(ids), len(x))
    clamped = 0
    for k, d in enumerate(ids):
        r = ref.resolve_row(observed, parent, rows, int(d))
        want = ref.density(x, grid, post[r], slope[r])
        assert np.array_equal(got[k], want), (k, d)
        clamped += int((ref.spline_interp(x, grid, post[r], slope[r]) < 0.0).sum())
        assert np.array_equal(got[k][3:8], post[r][[0, 1, 17, 98, 99]])      # at a knot: the knot
    assert clamped > 0 and got.min() == 0.0
    assert sum(1 for d in ids if not observed[d]) > 0


# ---- 4. / 5. the reference's own tests of this code -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree_states():
    """tests/hdpTests.c:109-190: the 8-process depth-3 tree, the reference's data without the points of DP 4, Gamma priors on the
    concentration parameters, execute_gibbs_sampling(10, 10, 10), finalize_distributions -- on the reference's grid and on a second one"""
    data = np.array(gzip.open(os.path.join(HDP_DATA, "test_hdp_data.txt.gz"), "rt").read().split(), dtype=np.float64)
    dps = np.array(gzip.open(os.path.join(HDP_DATA, "test_hdp_dps.txt.gz"), "rt").read().split(), dtype=np.int64)
    keep = dps != 4
    out = []
    for grid in ((-30.0, 30.0, 500), (-25.0, 35.0, 211)):
        s = sa.HdpState.new_tree([-1, 0, 0, 1, 1, 1, 2, 2], 3, grid, (0.0, 1.0, 2.0, 10.0), gamma_alpha=[1.0, 1.0, 2.0], gamma_beta=[0.2, 0.2, 0.1])
        s.pass_data(data[keep], dps[keep])
        s.gibbs(10, 10, 10, seed=7)
        s.finalize()
        out.append(s)
    yield out
    for s in out:
        s.close()


def test_distr_metrics_of_the_reference_test_hdp(tree_states):
    """add_distr_metric_tests / add_true_metric_tests (tests/hdpTests.c:70-107) over all 8 ids -- DP 4 has no data and walks to its
    parent: self-distance 0, non-negativity and symmetry within 1e-9 for the four metrics, the triangle inequality within 1e-4 for L2,
    Shannon-Jensen and Hellinger.  Properties, with the reference's constants: they do not depend on the sampler's draws."""
    s = tree_states[0]
    assert not s.array("observed")[4] and s.info.num_dps == 8
    ii, jj = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    for metric, r in METRICS:
        m = s.distance_pairs(metric, ii.ravel(), jj.ravel()).reshape(8, 8)
        assert not np.isnan(m).any()
        assert np.all(np.abs(np.diag(m)) <= 1e-9)
        assert np.all(m >= 0.0)
        assert np.all(np.abs(m - m.T) <= 1e-9)
        if r != ref.HELLINGER:
            assert m[4, 1] == 0.0 and m[1, 4] == 0.0          # two ids, one row
        if r == ref.KL:
            continue
        for i in range(6):
            for j in range(i + 1, 7):
                for k in range(j + 1, 8):
                    assert m[i, j] + m[j, k] >= m[i, k] - 1e-4, (metric, i, j, k)


def test_nhdp_distrs_of_the_reference(tmp_path):
    """tests/hdpTests.c:210-229: the flat ACGT 6-mer model over simple_alignment.tsv, 100 samples; KL between two k-mers is the same
    in both directions"""
    aln = str(tmp_path / "simple_alignment.tsv")
    open(aln, "w").write(gzip.open(os.path.join(HDP_DATA, "simple_alignment.tsv.gz"), "rt").read())
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_R73)
    s = sa.HdpState.new(sa.HDP_LAYOUT_FLAT, "ACGT", 6, (0.0, 100.0, 100), sa.hdp_nig_params_from_table(tab), gamma=[4.0, 20.0])
    assert s.pass_assignment_file(aln) == 1907
    s.gibbs(100, 0, 1, seed=3)
    s.finalize()
    for a, b in (("ACCCAA", "ATGATT"), ("GCACAT", "GGGGTA")):
        da, db = s.kmer_dp(a), s.kmer_dp(b)
        fwd, back = s.distance_pairs(sa.HDP_METRIC_KL, [da], [db])[0], s.distance_pairs(sa.HDP_METRIC_KL, [db], [da])[0]
        assert abs(fwd - back) <= 1e-9 and not np.isnan(fwd)
    s.close()


# ---- 6. two models ----------------------------------------------------------------------------------------------------------------
def _compare_want(s1, d1, s2, d2, r):
    g1, g2 = s1.array("grid"), s2.array("grid")
    row1 = [ref.resolve_row(s1.array("observed"), s1.array("dp_parent"), s1.array("row_of_dp"), int(d)) for d in d1]
    row2 = [ref.resolve_row(s2.array("observed"), s2.array("dp_parent"), s2.array("row_of_dp"), int(d)) for d in d2]
    post2, slope2 = s2.array("post"), s2.array("slope")
    second = np.array([ref.density(g1, g2, post2[q], slope2[q]) for q in row2])
    acc, s_abs = ref.integral(g1, s1.array("post")[row1], second, r)
    return ref.final(r, acc), acc, s_abs


def test_compare_a_state_with_itself(bundled, tree_states):
    """compare_hdp_distrs interpolates the second model on the first one's grid.  Where the truncated (x[i] - x[0]) / dx lands on i,
    t_left is exactly 0 and the interpolation at a knot returns the knot: then a state against itself is distance_pairs, bit for bit
    for L2.  That is so on the bundled model's grid (0, 100, 100) and on (-25, 35, 211); on (-30, 30, 500) the quotient falls just
    below i at 498 of the 500 knots, the reference's arithmetic then interpolates from the knot before with t_left just below 1, and
    some values differ from the knots in the last bits (78 of 500 for a Gaussian bump, by at most 1.4e-15) -- there the state against
    itself is held against the restatement instead."""
    s, grid, post, _ = bundled
    ids = np.array([s.kmer_dp(k) for k in ("ACEGOT", "TTTTTT", "GATACA", "OOOOOO", "CCGTAC", "AAAAAA")], dtype=np.int64)
    for st, a in ((s, ids), (tree_states[1], np.arange(8))):
        ii, jj = [v.ravel() for v in np.meshgrid(a, a, indexing="ij")]
        differ = ii != jj
        got = st.compare(st, ii, jj, sa.HDP_METRIC_L2)
        assert np.array_equal(got[differ], st.distance_pairs(sa.HDP_METRIC_L2, ii, jj)[differ])
        # no shortcut for equal ids: L2 of a row with itself is 0 by arithmetic, Hellinger is not
        assert np.all(got[~differ] == 0.0)
        own = st.array("post")[[ref.resolve_row(st.array("observed"), st.array("dp_parent"), st.array("row_of_dp"), int(d)) for d in a]]
        hell = ref.final(ref.HELLINGER, ref.integral(st.array("grid"), own, own, ref.HELLINGER)[0])
        assert np.array_equal(st.compare(st, a, a, sa.HDP_METRIC_HELLINGER), hell, equal_nan=True) and not np.any(hell == 0.0)
    st = tree_states[0]
    ii, jj = [v.ravel() for v in np.meshgrid(np.arange(8), np.arange(8), indexing="ij")]
    for metric, r in METRICS:
        dist, acc, s_abs = _compare_want(st, ii, st, jj, r)
        keep = (ii != jj) & ~((ii == 4) & (jj == 1)) & ~((ii == 1) & (jj == 4))     # (one row against itself: at the rounding floor)
        ref.check_against(r, st.compare(st, ii, jj, metric)[keep], dist[keep], acc[keep], s_abs[keep], label="500-point grid against itself")


def test_compare_two_states_on_different_grids(tree_states):
    """the synthetic tree finalised on (-30, 30, 500) and on (-25, 35, 211): each is the master in turn; the second model is read
    through its spline, beyond its grid through the spline's linear continuation, clamped at zero"""
    ii, jj = [v.ravel() for v in np.meshgrid(np.arange(8), np.arange(8), indexing="ij")]
    for first, second in ((tree_states[0], tree_states[1]), (tree_states[1], tree_states[0])):
        for metric, r in METRICS:
            got = first.compare(second, ii, jj, metric)
            dist, acc, s_abs = _compare_want(first, ii, second, jj, r)
            assert np.array_equal(np.isnan(got), np.isnan(dist))
            ok = ~np.isnan(dist)
            assert ok.all() or r != ref.L2
            if ok.any():
                ref.check_against(r, got[ok], dist[ok], acc[ok], s_abs[ok], label="two grids")


# ---- 7. the command-line tool -----------------------------------------------------------------------------------------------------
def test_compare_distributions_tool(bundled, tmp_path):
    s, grid, post, _ = bundled
    slope, observed, parent, rows = s.array("slope"), s.array("observed"), s.array("dp_parent"), s.array("row_of_dp")
    leaves = np.flatnonzero(parent == int(s.info.base_dp))
    alphabet, k = s.alphabet(), int(s.info.kmer_length)

    def name(dp):
        return "".join(alphabet[(int(dp) // len(alphabet) ** (k - 1 - q)) % len(alphabet)] for q in range(k))
    kmers = [name(d) for d in leaves[observed[leaves] == 1][[0, 5, 20, 77]]] + [name(leaves[observed[leaves] == 0][3])]
    assert [s.kmer_dp(km) for km in kmers] == [int(d) for d in leaves[observed[leaves] == 1][[0, 5, 20, 77]]] + [int(leaves[observed[leaves] == 0][3])]
    listing = tmp_path / "kmers.txt"
    listing.write_text("\n".join(kmers) + "\n")
    out_dir, dist_file = tmp_path / "distrs", tmp_path / "l2.tsv"
    out_dir.mkdir()
    pr = subprocess.run([TOOL, cases.NHDP, str(out_dir), "--kmers", str(listing), "--distances", "l2", "--out", str(dist_file)],
                        capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert pr.stderr.splitlines()[:2] == ["[compareDistributions] NOTICE: Loading NanoporeHDP from " + cases.NHDP,
                                          "[compareDistributions] NOTICE: Putting distributions in " + str(out_dir)]
    x = ref.linspace(30.0, 90.0, 600)
    assert (out_dir / "x_vals.txt").read_text() == "\n".join("%.17g" % v for v in x)        # (no newline behind the last value)
    assert sorted(os.listdir(str(out_dir))) == sorted(["x_vals.txt"] + [km + "_distr.txt" for km in kmers])
    r_of = [ref.resolve_row(observed, parent, rows, s.kmer_dp(km)) for km in kmers]
    assert r_of[4] == rows[int(s.info.base_dp)]
    for km, r in zip(kmers, r_of):
        want = ref.density(x, grid, post[r], slope[r])
        assert (out_dir / (km + "_distr.txt")).read_text() == "".join("%.17g\n" % v for v in want), km
    i, j = ref.tri_pairs(5)
    dist, _, _ = ref.all_pairs(grid, post[r_of], ref.L2)
    assert dist_file.read_text() == "".join("%s\t%s\t%.17g\n" % (kmers[a], kmers[b], d) for a, b, d in zip(i, j, dist))
    assert len(dist) == 10
