"""HDP distribution distances, what runs without a GPU: the numpy restatement the GPU tests compare against (tests/hdp_metric_ref.py)
on cases small enough to compute by hand, the argument checks of the new entry points (all of them come before any device use),
and the compareDistributions drop-in's handling of its command line."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import hdp_metric_ref as ref
import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "signalalign_amd", "bin", "compareDistributions")
SA_EINVAL, SA_ENODEVICE, SA_ESTATE = -1, -3, -7


def _one(metric, grid, p, q):
    acc, s = ref.integral(np.array(grid, dtype=np.float64), np.array([p], dtype=np.float64), np.array([q], dtype=np.float64), metric)
    return float(ref.final(metric, acc)[0]), float(acc[0]), float(s[0])


def test_restatement_on_two_point_cases():
    # L2: (p - q)^2 = 1, 1 over a step of 2
    assert _one(ref.L2, [0, 2], [1, 2], [2, 1])[:2] == (math.sqrt(2.0), 2.0)
    # Hellinger: sqrt(1/16) = 1/4 at both ends -> integral 1/2
    assert _one(ref.HELLINGER, [0, 2], [.25, .25], [.25, .25])[:2] == (math.sqrt(0.5), 0.5)
    # KL: 1 log(1/2) + 2 log 2 = log 2 at both ends (exact in binary: log(1/2) = -log 2) -> 2 log 2, and S = 3 log 2 per point
    d, acc, s = _one(ref.KL, [0, 2], [1, 2], [2, 1])
    assert d == acc == 2.0 * math.log(2.0) and s == 2.0 * (math.log(2.0) + 2.0 * math.log(2.0))
    # Shannon-Jensen: m = 2 at both ends
    pt = 0.5 * (1.0 * math.log(0.5) + 3.0 * math.log(1.5))
    d, acc, s = _one(ref.SHANNON_JENSEN, [0, 2], [1, 3], [3, 1])
    assert acc == 0.5 * (pt + pt) * 2.0 and d == math.sqrt(acc)
    assert s == 0.5 * (abs(math.log(0.5)) + abs(3.0 * math.log(1.5))) * 2.0      # (the log terms carry the point function's 0.5)


def test_restatement_on_three_point_cases():
    # a grid that is not equidistant: steps 1 and 2; (p - q)^2 = 1, 4, 9 -> 0.5 * 5 * 1 + 0.5 * 13 * 2
    assert _one(ref.L2, [0, 1, 3], [1, 2, 4], [0, 0, 1])[:2] == (math.sqrt(15.5), 15.5)
    # sqrt(p q) = 0, 1/2, 1/4 -> 0.5 * 0.5 * 1 + 0.5 * 0.75 * 2 = 1; the distance is sqrt(1 - 1) = 0
    assert _one(ref.HELLINGER, [0, 1, 3], [0, .5, .25], [7, .5, .25])[:2] == (0.0, 1.0)
    # the summation order is the grid's: 0.0 + a + b, not a + b in one go -- and the sum starts from 0.0
    pts = [2.0 * math.log(2.0) - math.log(2.0), 0.0, 3.0 * math.log(3.0) + math.log(1.0 / 3.0)]
    d, acc, _ = _one(ref.KL, [0, 1, 3], [1, 5, 3], [2, 5, 1])
    assert acc == (0.0 + 0.5 * (pts[0] + pts[1]) * 1.0) + 0.5 * (pts[1] + pts[2]) * 2.0 and d == acc


def test_restatement_ieee_specials():
    grid = [0.0, 0.5, 1.5]
    same = [0.3, 0.9, 0.1]
    for metric in (ref.KL, ref.SHANNON_JENSEN, ref.L2):
        assert _one(metric, grid, same, same)[0] == 0.0
    h = _one(ref.HELLINGER, grid, same, same)      # sqrt(1 - integral of p)
    assert h[0] == math.sqrt(1.0 - (0.5 * (0.3 + 0.9) * 0.5 + 0.5 * (0.9 + 0.1) * 1.0))
    zero = [0.3, 0.0, 0.1]
    assert math.isnan(_one(ref.KL, grid, zero, same)[0]) and math.isnan(_one(ref.SHANNON_JENSEN, grid, same, zero)[0])
    assert not math.isnan(_one(ref.L2, grid, zero, same)[0]) and not math.isnan(_one(ref.HELLINGER, grid, zero, same)[0])
    assert math.isnan(_one(ref.HELLINGER, grid, [2.0, 2.0, 2.0], [2.0, 2.0, 2.0])[0])      # an integral above one


def test_restatement_triangle_order_linspace_and_spline():
    i, j = ref.tri_pairs(4)
    assert list(zip(i, j)) == [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
    assert np.array_equal((i - 1) * i // 2 + j, np.arange(6))
    x = ref.linspace(30.0, 90.0, 600)
    dx = 60.0 / 599.0
    assert len(x) == 600 and x[0] == 30.0 and x[1] == 30.0 + 1 * dx and x[598] == 30.0 + 598 * dx and x[599] == 90.0
    # the spline through y = x^2 at 0, 1, 2 with slopes 0, 2, 4 is x^2 itself between the knots, a line outside
    kx, ky, ks = np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0, 4.0]), np.array([0.0, 2.0, 4.0])
    got = ref.spline_interp([-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0], kx, ky, ks)
    assert np.array_equal(got, [0.0, 0.0, 0.25, 1.0, 2.25, 4.0, 8.0])
    # dir_proc_density clamps at zero
    assert np.array_equal(ref.density([-1.0, 0.5], kx, ky, np.array([1.0, 2.0, 4.0])), [0.0, 0.375])


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def test_array_level_argument_checks_come_before_the_device():
    L = sa.lib()
    grid, rows, out = np.arange(3.0), np.ones((2, 3)), np.zeros(4)
    ms = C.c_double(-1.0)
    call = lambda g, n_g, r, n_r, metric, o: L.sa_hdp_distances(g, n_g, r, n_r, metric, 0, o, C.byref(ms))
    assert call(_dp(grid), 1, _dp(rows), 2, 0, _dp(out)) == SA_EINVAL                # grid_length < 2
    assert call(_dp(grid), 3, _dp(rows), 0, 0, _dp(out)) == SA_EINVAL                # n_rows < 1
    assert call(_dp(grid), 3, _dp(rows), 2, 4, _dp(out)) == SA_EINVAL                # unknown metric
    assert call(_dp(grid), 3, _dp(rows), 2, -1, _dp(out)) == SA_EINVAL
    assert call(None, 3, _dp(rows), 2, 0, _dp(out)) == SA_EINVAL                     # NULL arrays
    assert call(_dp(grid), 3, None, 2, 0, _dp(out)) == SA_EINVAL
    assert call(_dp(grid), 3, _dp(rows), 2, 0, None) == SA_EINVAL
    out[:] = 7.0
    assert call(_dp(grid), 3, _dp(rows), 1, 2, _dp(out)) == 0 and np.all(out == 7.0)  # one row: no pair, nothing written
    assert len(sa.hdp_distances(grid, rows[:1], sa.HDP_METRIC_L2)) == 0
    pair = lambda g, n_g, a, b, n, metric, o: L.sa_hdp_distances_paired(g, n_g, a, b, n, metric, 0, o, None)
    assert pair(_dp(grid), 1, _dp(rows), _dp(rows), 2, 0, _dp(out)) == SA_EINVAL
    assert pair(_dp(grid), 3, _dp(rows), _dp(rows), 0, 0, _dp(out)) == SA_EINVAL
    assert pair(_dp(grid), 3, _dp(rows), _dp(rows), 2, 9, _dp(out)) == SA_EINVAL
    assert pair(_dp(grid), 3, None, _dp(rows), 2, 0, _dp(out)) == SA_EINVAL
    assert pair(_dp(grid), 3, _dp(rows), None, 2, 0, _dp(out)) == SA_EINVAL
    assert pair(None, 3, _dp(rows), _dp(rows), 2, 0, _dp(out)) == SA_EINVAL
    assert pair(_dp(grid), 3, _dp(rows), _dp(rows), 2, 0, None) == SA_EINVAL
    if sa.device_count() == 0:
        assert call(_dp(grid), 3, _dp(rows), 2, 0, _dp(out)) == SA_ENODEVICE
        assert pair(_dp(grid), 3, _dp(rows), _dp(rows), 2, 0, _dp(out)) == SA_ENODEVICE


def test_state_level_argument_checks_come_before_the_device():
    L = sa.lib()
    s = sa.HdpState(cases.NHDP)
    n_dps = int(s.info.num_dps)
    ids, bad_hi, bad_lo = np.array([0, 1], dtype=np.int64), np.array([0, n_dps], dtype=np.int64), np.array([-1, 0], dtype=np.int64)
    x, out = np.array([50.0, 60.0]), np.zeros(8)
    for bad in (bad_hi, bad_lo):
        assert L.sa_hdp_state_densities(s._h, _ip(bad), 2, _dp(x), 2, 0, _dp(out)) == SA_EINVAL
        assert L.sa_hdp_state_distance_pairs(s._h, 0, _ip(bad), _ip(ids), 2, 0, _dp(out)) == SA_EINVAL
        assert L.sa_hdp_state_distance_pairs(s._h, 0, _ip(ids), _ip(bad), 2, 0, _dp(out)) == SA_EINVAL
        assert L.sa_hdp_state_compare(s._h, _ip(bad), s._h, _ip(ids), 2, 0, 0, _dp(out)) == SA_EINVAL
        assert L.sa_hdp_state_compare(s._h, _ip(ids), s._h, _ip(bad), 2, 0, 0, _dp(out)) == SA_EINVAL
    assert L.sa_hdp_state_distances(s._h, 4, 0, _dp(out), None) == SA_EINVAL
    assert L.sa_hdp_state_distances(s._h, 0, 0, None, None) == SA_EINVAL
    assert L.sa_hdp_state_distance_pairs(s._h, 7, _ip(ids), _ip(ids), 2, 0, _dp(out)) == SA_EINVAL
    assert L.sa_hdp_state_distance_pairs(s._h, 0, None, _ip(ids), 2, 0, _dp(out)) == SA_EINVAL
    assert L.sa_hdp_state_compare(s._h, _ip(ids), None, _ip(ids), 2, 0, 0, _dp(out)) == SA_EINVAL
    assert L.sa_hdp_state_densities(s._h, _ip(ids), 2, None, 2, 0, _dp(out)) == SA_EINVAL
    assert L.sa_hdp_state_densities(None, _ip(ids), 2, _dp(x), 2, 0, _dp(out)) == SA_EINVAL
    assert s.alphabet() == "ACEGOT"
    # a model whose splines are not finalised: SA_ESTATE from every state-level call
    raw = sa.HdpState.new(sa.HDP_LAYOUT_FLAT, "ACGT", 3, (0.0, 100.0, 50), (60.0, 1.0, 2.0, 10.0), gamma=[1.0, 1.0])
    assert raw.info.splines_finalized == 0
    assert L.sa_hdp_state_densities(raw._h, _ip(ids), 2, _dp(x), 2, 0, _dp(out)) == SA_ESTATE
    assert L.sa_hdp_state_distances(raw._h, 0, 0, _dp(out), None) == SA_ESTATE
    assert L.sa_hdp_state_distance_pairs(raw._h, 0, _ip(ids), _ip(ids), 2, 0, _dp(out)) == SA_ESTATE
    assert L.sa_hdp_state_compare(s._h, _ip(ids), raw._h, _ip(ids), 2, 0, 0, _dp(out)) == SA_ESTATE
    assert L.sa_hdp_state_compare(raw._h, _ip(ids), s._h, _ip(ids), 2, 0, 0, _dp(out)) == SA_ESTATE
    if sa.device_count() == 0:
        for call in (lambda: s.densities(ids, x), lambda: s.distances(sa.HDP_METRIC_L2), lambda: s.distance_pairs(sa.HDP_METRIC_KL, ids, ids[::-1]),
                     lambda: s.compare(s, ids, ids, sa.HDP_METRIC_HELLINGER)):
            with pytest.raises(sa.SaError) as ei:
                call()
            assert ei.value.code == SA_ENODEVICE
    raw.close()
    s.close()


def test_compare_distributions_command_line(tmp_path):
    usage = "USAGE_NEW: compareDistributions [NanoporeHDP_file] [distribution_directory]\n"
    for argv in ([], [cases.NHDP], [cases.NHDP, str(tmp_path), "extra"], [cases.NHDP, "--kmers", "x"]):
        pr = subprocess.run([TOOL] + argv, capture_output=True, text=True, timeout=60)
        assert pr.returncode == 1 and pr.stderr == usage and pr.stdout == "", argv
    # the two notices come first, then the model is read: a k-mer outside the alphabet, a model that is not finalised
    km = tmp_path / "kmers.txt"
    km.write_text("ACEGOT\nACGTNA\n")
    pr = subprocess.run([TOOL, cases.NHDP, str(tmp_path), "--kmers", str(km)], capture_output=True, text=True, timeout=60)
    lines = pr.stderr.splitlines()
    assert pr.returncode == 1 and lines[0] == "[compareDistributions] NOTICE: Loading NanoporeHDP from " + cases.NHDP
    assert lines[1] == "[compareDistributions] NOTICE: Putting distributions in " + str(tmp_path)
    assert "ACGTNA" in lines[2] and "outside alphabet" in lines[2]
    raw = sa.HdpState.new(sa.HDP_LAYOUT_FLAT, "ACGT", 3, (0.0, 100.0, 50), (60.0, 1.0, 2.0, 10.0), gamma=[1.0, 1.0])
    path = str(tmp_path / "raw.nhdp")
    raw.write(path)
    raw.close()
    pr = subprocess.run([TOOL, path, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "finalize" in pr.stderr.splitlines()[2]
    assert not os.path.exists(str(tmp_path / "x_vals.txt"))
    pr = subprocess.run([TOOL, cases.NHDP, str(tmp_path), "--distances", "euclid", "--out", str(tmp_path / "d.tsv")], capture_output=True,
                        text=True, timeout=60)
    assert pr.returncode == 1 and "euclid" in pr.stderr
