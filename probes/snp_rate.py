"""Single-nucleotide probabilities on the device: BASELINE configs[1]-shaped synthetic reads (R9.4 6-mer Gaussian, --reads x
--events) become --step jobs each, job s with X (= ACGT) at the reference positions = s (mod step), all in one batch with
SA_FLAG_POSITION_CALLS.  Prints one JSON line: jobs, pairs, the batch's device time, sa_batch_position_calls' kernel time (HIP
events) and its share, the ring regions, and the distribution of rows per position (the bucket sizes)."""
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
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--step", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")
    pm = sa.Model.load(model)
    reads = synth.make_reads_parallel(dict(kind="gauss", model=model, events=a.events, kw={}), list(range(a.reads)))
    jobs = []
    for r in reads:
        for s in range(a.step):
            ref = list(r["ref"])
            for i in range(s, len(ref), a.step):
                ref[i] = "X"
            jobs.append(dict(r, ref="".join(ref)))
    p = sa.default_params(threshold=0.01, expansion=50, trace_back=100)
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig({"X": "ACGT"}), flags=sa.FLAG_POSITION_CALLS)
    b.run()
    st = b.stats()
    first = np.zeros(len(jobs) + 1, dtype=np.int64)
    n_pairs = int(b.results_view(first)[1][-1])
    ms = []
    for _ in range(a.repeats):
        info = {}
        calls = b.position_calls(stats=info)
        ms.append(info["kernel_ms"])
    rows = np.concatenate([c["n_rows"] for c in calls])
    cells = st.cells_forward + st.cells_backward
    print(json.dumps(dict(reads=a.reads, events=a.events, step=a.step, jobs=len(jobs), pairs=n_pairs, positions=int(len(rows)),
                          batch_device_ms=round(st.ms_total_device, 2), n_chunks=int(st.n_chunks),
                          ring_regions=int(st.n_ring_regions), regions=int(st.n_regions),
                          cell_paths_per_s=round(cells / (st.ms_total_device * 1e-3), 1),
                          position_kernel_ms=[round(x, 3) for x in ms],
                          share_of_batch_device=round(min(ms) / st.ms_total_device, 4),
                          rows_per_position=dict(mean=round(float(rows.mean()), 2), p50=int(np.percentile(rows, 50)),
                                                 p90=int(np.percentile(rows, 90)), p99=int(np.percentile(rows, 99)),
                                                 max=int(rows.max())))), flush=True)
    b.close()


if __name__ == "__main__":
    main()
