"""Marginals over reads on the device, on the workload of probes/snp_rate.py: --reads x --events configs[1]-shaped synthetic
reads become --step jobs each (X at the positions = s (mod step)), one batch with SA_FLAG_POSITION_CALLS; the reads are laid on
one contig --spacing bases apart, every other one mapped backward.  Prints one JSON line and writes it to --out:
  position_kernel_ms     sa_batch_position_calls, the yardstick, re-measured here
  add_batch_fold_ms      the position fold inside sa_snp_marginals_add_batch (the code the two share)
  add_batch_extra_ms     what add_batch runs beyond it: window, rows, buckets, sort, fold
  finish_ms              sa_snp_marginals_finish
  pcie_bytes             with --snp-dir (every position call as sa_position_call_t) and without (the job map and the slot table up, the sites down)
  cpu_restatement_s      tests/snp_marginals_ref.py over the rows of the first --cpu-reads reads, one thread, and the same scaled
                         to all rows
Each device time is the smallest of --repeats calls after one warm-up call."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import signalalign_amd as sa  # noqa: E402
from signalalign_amd import _capi, synth  # noqa: E402
import snp_marginals_ref as ref  # noqa: E402

K = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--step", type=int, default=10)
    ap.add_argument("--spacing", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-reads", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snp_marginals.json"))
    a = ap.parse_args()
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")
    pm = sa.Model.load(model)
    reads = synth.make_reads_parallel(dict(kind="gauss", model=model, events=a.events, kw={}), list(range(a.reads)))
    jobs, job_map = [], []
    contig_len = a.spacing * a.reads + max(len(r["ref"]) for r in reads) + a.step
    for i, r in enumerate(reads):
        n, lo, same = len(r["ref"]), a.spacing * i, i % 2 == 0
        pos0, sign = (lo, 1) if same else (lo + n - 1, -1)
        for s in range(a.step):
            jobs.append(dict(r, ref=sa.snp_substitute(r["ref"], pos0, not same, a.step, s)))
            job_map.append(dict(contig=0, pos0=pos0, pos_sign=sign, x0=lo if same else lo + n - K, x_sign=sign, strand=0,
                                direction=int(same), run=i, group=i * a.step + s))
    p = sa.default_params(threshold=0.01, expansion=50, trace_back=100)
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig({"X": "ACGT"}), flags=sa.FLAG_POSITION_CALLS)
    b.run()
    st = b.stats()
    pos_ms = []
    for _ in range(a.repeats + 1):   # (the C entry point itself: the Python wrapper's per-record conversion is not what is timed)
        ptrs = (C.POINTER(_capi.PositionCall) * len(jobs))()
        cnt = np.zeros(len(jobs), dtype=np.int64)
        kms = C.c_double()
        rc = sa.lib().sa_batch_position_calls(b._h, 0, ptrs, cnt.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(kms))
        assert rc == 0, rc
        for q in ptrs:
            sa.lib().sa_free(q)
        pos_ms.append(kms.value)
    calls = b.position_calls()
    n_positions = int(sum(len(c["p"]) for c in calls))
    fold_ms, extra_ms, fin_ms, table = [], [], [], None
    for _ in range(a.repeats + 1):
        t = sa.SnpMarginals([contig_len], step=a.step)
        info, fin = {}, {}
        t.add_batch(b, job_map, stats=info)
        table = t.finish(stats=fin)
        t.close()
        fold_ms.append(info["kernel_ms_position_fold"])
        extra_ms.append(info["kernel_ms"])
        fin_ms.append(fin["kernel_ms"])
    # the restatement over the rows of the first reads, as a user reading the per-read files back would run it
    rows = []
    for j in range(min(a.cpu_reads, a.reads) * a.step):
        c, m = calls[j], job_map[j]
        if not len(c["p"]):
            continue
        idx = [m["x0"] + m["x_sign"] * c["x_min"], m["x0"] + m["x_sign"] * c["x_max"]]
        w_lo, w_hi = sa.snp_site_window(min(idx), max(idx), a.step)
        for q, pq in enumerate(c["p"].tolist()):
            pos = m["pos0"] + m["pos_sign"] * pq
            if w_lo <= pos < w_hi:
                letters = c["letters"][q]
                rows.append((0, pos, m["run"], 0, m["direction"], tuple(float(c["prob"][q][letters.index(l)]) for l in "ACGT")))
    t0 = time.perf_counter()
    ref.finish(ref.accumulate([rows]))
    cpu_s = time.perf_counter() - t0
    n_rows = int(table["depth"].sum())
    out = dict(reads=a.reads, events=a.events, step=a.step, jobs=len(jobs), positions=n_positions, rows_added=n_rows,
               sites=int(len(table)), depth=dict(mean=round(float(table["depth"].mean()), 2), max=int(table["depth"].max())),
               batch_device_ms=round(st.ms_total_device, 2),
               position_kernel_ms=[round(x, 3) for x in pos_ms[1:]],
               add_batch_fold_ms=[round(x, 3) for x in fold_ms[1:]],
               add_batch_extra_ms=[round(x, 3) for x in extra_ms[1:]],
               finish_ms=[round(x, 3) for x in fin_ms[1:]],
               extra_share_of_position_fold=round(min(extra_ms[1:]) / min(pos_ms[1:]), 4),
               pcie_bytes=dict(with_snp_dir=n_positions * C.sizeof(_capi.PositionCall),
                               without_snp_dir=len(jobs) * C.sizeof(_capi.SnpJobMap) + 4 * n_positions
                               + int(len(table)) * _capi.SNP_MARGINAL_DTYPE.itemsize),
               cpu_restatement_s=dict(rows=len(rows), seconds=round(cpu_s, 3),
                                      scaled_to_all_rows=round(cpu_s * n_rows / max(len(rows), 1), 1)))
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
