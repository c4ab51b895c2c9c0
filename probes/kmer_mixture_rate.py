"""Kernel time of one sa_kmer_table_mixture call at K = 2 (HIP events: the gather and sort of the long segments and the EM kernel),
median of 5 calls after 2 warm-ups, and next to it the time sklearn's GaussianMixture takes for the same fits from the same
start on one CPU thread of the same machine (the figure the device fit replaces).
  (a) 4096 k-mers x 1000 rows: every segment is sorted and kept in LDS
  (b) the canonical k-mers of the two CCWGG motif pairs (CCAGG:CEAGG, CCTGG:CETGG; 6-mers) x 10 000 rows: every segment is
      sorted by rocPRIM in HBM and streamed once per iteration
Rows are a planted pair 0.4 N(78, 1.2) + 0.6 N(84, 1.5) per k-mer.  Prints one JSON line per case; --out appends them to a file
(profiles/kmer_mixture_rate.jsonl)."""
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
import kmer_mixture_ref as ref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "models")


def measure(name, model_path, ids, rows_per_kmer, sklearn_fits):
    pm = sa.Model.load(model_path)
    rng = np.random.default_rng(1)
    n = len(ids) * rows_per_kmer
    low = rng.random(n) < 0.4
    x = np.round(np.where(low, 78.0 + 1.2 * rng.standard_normal(n), 84.0 + 1.5 * rng.standard_normal(n)), 6)
    km = np.repeat(np.asarray(ids, dtype=np.int32), rows_per_kmer)
    order = rng.permutation(n)
    tab = sa.KmerTable(pm, rows_per_kmer, 0.0)
    tab.add_rows(km[order], x[order], np.round(rng.uniform(0.5, 1.0, n), 6))
    ms = []
    for _ in range(7):
        info = {}
        fits = tab.mixture(ids, n_components=2, info=info)
        ms.append(info["kernel_ms"])
    assert int((fits["status"] == 0).sum()) == len(ids) and bool(fits["converged"].all())
    out = dict(case=name, kmers=len(ids), rows_per_kmer=rows_per_kmer, K=2, kernel_ms_median_of_5=round(float(np.median(ms[2:])), 3),
               kernel_ms_all=[round(v, 3) for v in ms], mean_iterations=round(float(fits["n_iter"].mean()), 2))
    try:
        from threadpoolctl import threadpool_limits
        import sklearn  # noqa: F401
    except ImportError:
        sklearn_fits = 0
    if sklearn_fits:
        rows = tab.rows(0)
        by = {int(k): rows["descaled_units"][rows["kmer_id"] == k] / 1e6 for k in ids[:sklearn_fits]}
        with threadpool_limits(limits=1):
            t0 = time.perf_counter()
            for k in ids[:sklearn_fits]:
                ref.sklearn_fit(by[int(k)], 2, 100, 1e-3)
            dt = time.perf_counter() - t0
        out.update(sklearn_fits_timed=len(by), sklearn_one_thread_s=round(dt, 3),
                   sklearn_one_thread_s_scaled_to_all_kmers=round(dt * len(ids) / len(by), 3))
    tab.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sklearn-fits", type=int, default=256, help="fits timed with sklearn per case (0: none); scaled to the case")
    a = ap.parse_args()
    cpg = os.path.join(GOLD, "testModelR9.4_450bps.cpg.6mer.template.model")
    pm = sa.Model.load(cpg)
    pairs = sorted(set(sa.motif_kmer_pairs(6, "CCAGG", "CEAGG") + sa.motif_kmer_pairs(6, "CCTGG", "CETGG")))
    motif_ids = sorted(set(pm.kmer_id(c) for c, _ in pairs))
    lines = [measure("a_4096x1000_lds", os.path.join(GOLD, "testModelR9.4_450bps.nucleotide.6mer.template.model"),
                     list(range(4096)), 1000, a.sklearn_fits),
             measure("b_ccwgg_x10000_streamed", cpg, motif_ids, 10000, a.sklearn_fits)]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
