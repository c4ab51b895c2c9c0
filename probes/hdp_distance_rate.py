"""Rate of sa_hdp_distances (all pairs among the k-mer distributions of an HDP, signalalign_amd/csrc/sa_hdpdist.hip) at the size of the
CpG 6-mer model: --rows synthetic rows (15 625 = 5^6 leaves) x --grid points (400), once per metric after a small warm-up call.
One JSON line per metric: kernel_ms (HIP events around the kernels alone), pair-points/s over it, wall time of the whole call (upload,
kernels, the triangle's transfer in bands and its copy into ordinary memory) -- and, unless --no-cpu, the same formulas in numpy on
a --cpu-rows subset (2000), SCALED by the pair count to the full problem: an extrapolation, labelled as one.
Under `rocprofv3 --kernel-trace --stats -- python probes/hdp_distance_rate.py --no-cpu` the per-kernel statistics."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import signalalign_amd as sa  # noqa: E402

NAMES = {sa.HDP_METRIC_KL: "kl", sa.HDP_METRIC_HELLINGER: "hellinger", sa.HDP_METRIC_L2: "l2", sa.HDP_METRIC_SHANNON_JENSEN: "shannon_jensen"}


def synthetic_rows(n_rows, grid_length, seed=1):
    """densities as a finalised HDP holds them: two-component Gaussian mixtures on linspace(30, 90), strictly positive"""
    rng = np.random.default_rng(seed)
    grid = np.linspace(30.0, 90.0, grid_length)
    m1, m2 = rng.uniform(40.0, 80.0, size=(2, n_rows, 1))
    s1, s2 = rng.uniform(1.0, 6.0, size=(2, n_rows, 1))
    w = rng.uniform(0.2, 0.8, size=(n_rows, 1))
    gauss = lambda m, s: np.exp(-0.5 * ((grid[None, :] - m) / s) ** 2) / (s * np.sqrt(2.0 * np.pi))
    return grid, np.ascontiguousarray(w * gauss(m1, s1) + (1.0 - w) * gauss(m2, s2) + 1e-6)


def numpy_all_pairs(grid, rows, metric, block=64):
    """the reference's formulas, vectorised over pairs in blocks of first rows, sequential over the grid"""
    n = rows.shape[0]
    dx = np.diff(grid)
    cols = np.ascontiguousarray(rows.T)             # grid point x row: a grid step reads contiguous pairs
    out = np.empty(n * (n - 1) // 2)
    with np.errstate(all="ignore"):
        for i0 in range(1, n, block):
            i = np.arange(i0, min(i0 + block, n))
            ii = np.repeat(i, i)
            jj = np.concatenate([np.arange(k) for k in i])
            p, q = cols[:, ii], cols[:, jj]
            if metric == sa.HDP_METRIC_KL:
                pt = p * np.log(p / q) + q * np.log(q / p)
            elif metric == sa.HDP_METRIC_HELLINGER:
                pt = np.sqrt(p * q)
            elif metric == sa.HDP_METRIC_L2:
                pt = (p - q) * (p - q)
            else:
                m = 0.5 * (p + q)
                pt = 0.5 * (p * np.log(p / m) + q * np.log(q / m))
            acc = np.zeros(len(ii))
            for g in range(1, len(grid)):
                acc += 0.5 * (pt[g - 1] + pt[g]) * dx[g - 1]
            first = (i0 - 1) * i0 // 2
            out[first:first + len(ii)] = acc if metric == sa.HDP_METRIC_KL else np.sqrt(1.0 - acc if metric == sa.HDP_METRIC_HELLINGER else acc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=15625)
    ap.add_argument("--grid", type=int, default=400)
    ap.add_argument("--cpu-rows", type=int, default=2000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--metrics", nargs="+", default=["kl", "hellinger", "l2", "shannon_jensen"])
    a = ap.parse_args()
    if sa.device_count() < 1:
        raise SystemExit("hdp_distance_rate: no GPU; nothing is measured without one")
    grid, rows = synthetic_rows(a.rows, a.grid)
    pairs = a.rows * (a.rows - 1) // 2
    sa.hdp_distances(grid, rows[:512], sa.HDP_METRIC_L2)          # code objects loaded, scratch allocated below the timed calls' size
    for metric, name in NAMES.items():
        if name not in a.metrics:
            continue
        sa.hdp_distances(grid, rows[:512], metric)
        stats = {}
        t0 = time.perf_counter()
        got = sa.hdp_distances(grid, rows, metric, stats=stats)
        wall = time.perf_counter() - t0
        t0 = time.perf_counter()
        again = sa.hdp_distances(grid, rows, metric)              # (scratch and pinned buffers now at their final size)
        wall_warm = time.perf_counter() - t0
        line = dict(metric=name, rows=a.rows, grid_length=a.grid, pairs=pairs, pair_points=pairs * a.grid,
                    kernel_ms=round(stats["kernel_ms"], 2), pair_points_per_s=round(pairs * a.grid / (stats["kernel_ms"] * 1e-3), -6),
                    wall_s_first_call=round(wall, 3), wall_s=round(wall_warm, 3), output_gb=round(pairs * 8 / 1e9, 3),
                    nan=int(np.isnan(got).sum()), same_bits_twice=bool(np.array_equal(got, again, equal_nan=True)))
        if not a.no_cpu:
            n = min(a.cpu_rows, a.rows)
            t0 = time.perf_counter()
            want = numpy_all_pairs(grid, rows[:n], metric)
            cpu_s = time.perf_counter() - t0
            sub = n * (n - 1) // 2
            err = np.abs(got[:sub] - want)
            line.update(cpu_rows=n, cpu_numpy_s_subset=round(cpu_s, 2), cpu_numpy_s_extrapolated_to_all_pairs=round(cpu_s * pairs / sub, 1),
                        cpu_note="numpy on the subset, scaled by the pair count: an extrapolation, not a measurement of the full problem",
                        max_abs_diff_vs_numpy_on_subset=float(np.nanmax(err)))
        print(json.dumps(line), flush=True)
    sa.hdp_distances_release()


if __name__ == "__main__":
    main()
