"""Kernel time of sa_kmer_table_add_batch (the top-N selection of the Gaussian emission training) on BASELINE-shaped batches:
--config 1 (R9.4 6-mer Gaussian, 2000 x 5000 events), 2 (R9.4 6-mer CpG model, every CpG cytosine C/E, 10 000 reads) or 3 (HDP
emissions, templateSingleLevelFixed.nhdp, 5000 reads, threshold 0.01).  For each N of --n: one table, the batch added
--repeats times (the later adds merge against a full table), and the statistics kernel.  Prints one JSON line per N: pairs,
the batch's device step, add_batch and stats kernel times (HIP events, device work only)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import signalalign_amd as sa  # noqa: E402
from signalalign_amd import synth  # noqa: E402


def main():
    # (the read generator spawns worker processes that import this file: everything runs under the __main__ guard)
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=[1, 2, 3])
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--n", type=int, nargs="+", default=[10, 10000])
    ap.add_argument("--min-prob", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    gold = os.path.join(ROOT, "tests", "golden", "models")
    ambig, nhdp, threshold = None, None, 0.01
    if a.config == 1:
        model, reads, kw = os.path.join(gold, "testModelR9.4_450bps.nucleotide.6mer.template.model"), 2000, {}
    elif a.config == 2:
        model, reads, kw = os.path.join(gold, "testModelR9.4_450bps.cpg.6mer.template.model"), 10000, {"cpg_ambiguous": True}
        ambig = sa.default_ambig({"X": "CE"})
    else:
        model, reads, kw = os.path.join(gold, "testModelR73_acegot_template.model"), 5000, {}
        nhdp = os.path.join(gold, "templateSingleLevelFixed.nhdp")
    reads = a.reads or reads
    pm = sa.Model.load(model, nhdp)
    if nhdp:
        pm.set_to_hdp_expected_values()
        spec = dict(kind="hdp", model=model, nhdp=nhdp, events=a.events, table5=np.array(pm.table5()),
                    ref_pool=os.path.join(ROOT, "tests", "golden", "npReads", "ZymoRef.txt"))
    else:
        spec = dict(kind="gauss", model=model, events=a.events, kw=kw)
    jobs = synth.make_reads_parallel(spec, list(range(reads)))
    p = sa.default_params(threshold=threshold, expansion=50, trace_back=100)
    b = sa.Batch(pm, p, jobs, ambig=ambig if ambig is not None else sa.default_ambig())
    b.run()
    first = np.zeros(len(jobs) + 1, dtype=np.int64)
    n_pairs = int(b.results_view(first)[1][-1])
    bst = b.stats()
    for n in a.n:
        tab = sa.KmerTable(pm, n, a.min_prob)
        add_ms = []
        for _ in range(a.repeats):
            info = {}
            tab.add_batch(b, 0, stats=info)
            add_ms.append(info["kernel_ms"])
        info = {}
        tab.stats(0, info=info)
        stats_ms = info["kernel_ms"]
        tab.stats(0, use_median=True, info=info)
        kept = len(tab.rows(0))
        tab.close()
        print(json.dumps(dict(config=a.config, reads=reads, events=a.events, threshold=threshold, pairs=n_pairs, N=n,
                              min_prob=a.min_prob, kept_rows=kept, step_device_ms=round(bst.ms_total_device, 2),
                              add_batch_kernel_ms=[round(x, 3) for x in add_ms], stats_kernel_ms=round(stats_ms, 3),
                              stats_median_kernel_ms=round(info["kernel_ms"], 3),
                              share_of_device_step=round(min(add_ms) / bst.ms_total_device, 4))), flush=True)
    b.close()


if __name__ == "__main__":
    main()
