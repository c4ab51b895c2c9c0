"""Time of sa_kmer_table_kde for every k-mer of the R9.4 6-mer model (4096) at 1000 and at 10 000 synthetic rows per k-mer, on
linspace(30, 90, 600) and on 1200 points, bandwidth 0.5: the HIP-event kernel time (gather, sort and KDE kernels) and the time
of the whole call (with the chunked copy of the 4096 x n_x block into ordinary host memory), each the median of 3 calls after a
warm-up; the kernel time again with SA_KDE_NO_SKIP=1 (every exp evaluated, same bits), i.e. without the wave-level skip.
Rows of a k-mer are N(level mean, 1.5 pA).  Beside it the numpy restatement (tests/kde_ref.py) on one CPU thread for a few
k-mers, scaled to all of them: an extrapolation, not a measurement of the full problem.  Writes profiles/kmer_kde.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import signalalign_amd as sa  # noqa: E402
import kde_ref as ref  # noqa: E402

MODEL = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")


def timed(tab, x, env):
    for k, v in env.items():
        os.environ[k] = v
    kernel, call = [], []
    out = None
    for _ in range(4):
        info = {}
        t0 = time.perf_counter()
        out = tab.kde(x, None, bandwidth=0.5, info=info)
        call.append(time.perf_counter() - t0)
        kernel.append(info["kernel_ms"])
    for k in env:
        del os.environ[k]
    return out, round(float(np.median(kernel[1:])), 3), round(float(np.median(call[1:])) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmer_kde.json"))
    ap.add_argument("--cpu-kmers", type=int, default=8)
    ap.add_argument("--rows", type=int, nargs="*", default=[1000, 10000])
    a = ap.parse_args()
    pm = sa.Model.load(MODEL)
    level = pm.table5().reshape(-1, 5)[:, 0].copy()
    nk = len(level)
    cases = []
    for rows_per_kmer in a.rows:
        rng = np.random.default_rng(rows_per_kmer)
        n = nk * rows_per_kmer
        km = np.repeat(np.arange(nk, dtype=np.int32), rows_per_kmer)
        v = np.round(level[km] + 1.5 * rng.standard_normal(n), 6)
        order = rng.permutation(n)
        tab = sa.KmerTable(pm, rows_per_kmer, 0.0)
        tab.add_rows(km[order], v[order], np.round(rng.uniform(0.5, 1.0, n), 6))
        del v, order
        for n_x in (600, 1200):
            x = np.linspace(30.0, 90.0, n_x)
            out, kernel_ms, call_ms = timed(tab, x, {})
            out2, kernel_ms_no_skip, _ = timed(tab, x, {"SA_KDE_NO_SKIP": "1"})
            case = dict(kmers=nk, rows_per_kmer=rows_per_kmer, n_x=n_x, bandwidth=0.5, row_points=nk * rows_per_kmer * n_x,
                        kernel_ms=kernel_ms, call_ms=call_ms, kernel_ms_without_wave_skip=kernel_ms_no_skip,
                        same_bits_with_and_without_skip=bool(out.tobytes() == out2.tobytes()),
                        output_mb=round(out.nbytes / 1e6, 1), all_finite=bool(np.isfinite(out).all()))
            if a.cpu_kmers and rows_per_kmer == a.rows[0]:
                rows = tab.rows(0)
                ids = list(range(0, nk, nk // a.cpu_kmers))[:a.cpu_kmers]
                by = {k: rows["descaled_units"][rows["kmer_id"] == k] for k in ids}
                t0 = time.perf_counter()
                worst = 0.0
                for k in ids:
                    e = ref.kde_log_density(by[k], x, 0.5)
                    worst = max(worst, float((np.abs(out[k] - e) / np.maximum(1.0, np.abs(e))).max()))
                dt = time.perf_counter() - t0
                case.update(cpu_kmers=len(ids), cpu_numpy_s_subset=round(dt, 3),
                            cpu_numpy_s_extrapolated_to_all_kmers=round(dt * nk / len(ids), 1),
                            cpu_note="the numpy restatement on one thread for the subset, scaled by the k-mer count: an extrapolation, "
                                     "not a measurement of the full problem",
                            max_rel_diff_vs_numpy_on_subset=worst)
            print(json.dumps(case), flush=True)
            cases.append(case)
        tab.close()
    meta = dict(what="sa_kmer_table_kde over all 4096 k-mers of the R9.4 6-mer model, one MI355X, one visit",
                made_by=["python probes/kmer_kde_rate.py"],
                note="kernel_ms: HIP events around the gather, sort and KDE kernels, median of 3 calls after a warm-up; call_ms: the whole "
                     "call, output copied in chunks into ordinary memory; kernel_ms_without_wave_skip: SA_KDE_NO_SKIP=1")
    with open(a.out, "w") as f:
        json.dump(dict(_meta=meta, rate=cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
