"""Guide deviation on the device, on a configs[1]-shaped batch: --reads x --events synthetic reads in one batch, their anchors the
guide, the MEA paths of sa_batch_mea handed in as the CLI hands them in.  Prints one JSON line and writes it to --out:
  deviation_window_ms    kernel_ms of sa_batch_guide_deviation with the LDS window (SA_DEV_WINDOW)
  deviation_direct_ms    the same call as it runs by default (SA_DEV_DIRECT): every record a global 64-bit atomic maximum -- the A/B
                         of the window, in this one process, the two alternating
  batch_device_ms        the batch's own step time, and mea_kernel_ms that of the paths, beside them
  pcie_bytes             what crosses PCIe for the stage (jobs, anchors and path events up; summaries, histograms and sets down)
                         against the bytes of the full TSV the script would have read (estimated from the rows of the first
                         --cpu-reads reads, formatted as the CLI does)
  cpu_restatement_s      tests/deviation_ref.py over the first --cpu-reads reads, one thread, and the same EXTRAPOLATED to all records
Each device time is the smallest of --repeats calls after one warm-up call."""
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
from signalalign_amd import synth  # noqa: E402
import deviation_ref as ref  # noqa: E402

K = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-reads", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_deviation.json"))
    a = ap.parse_args()
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")
    pm = sa.Model.load(model)
    reads = synth.make_reads_parallel(dict(kind="gauss", model=model, events=a.events, kw={}), list(range(a.reads)))
    b = sa.Batch(pm, sa.default_params(threshold=0.01, expansion=50, trace_back=100), reads)
    b.run()
    st = b.stats()
    mea_info = {}
    paths = [m[0] for m in b.mea(stats=mea_info)]
    rows, first = b.pairs_all()
    n_records = int(first[-1])
    djobs = [dict(ax=r["ax"], ay=r["ay"], n_events=len(r["events"])) for r in reads]
    ms = {sa.DEV_WINDOW: [], sa.DEV_DIRECT: []}
    got = {}
    for _ in range(a.repeats + 1):
        for flags in (sa.DEV_WINDOW, sa.DEV_DIRECT):
            got[flags] = sa.batch_guide_deviation(b, djobs, mea=paths, flags=flags)
            ms[flags].append(got[flags]["kernel_ms"])
    for f in ("reads", "sets", "hist", "total_hist"):
        assert got[sa.DEV_WINDOW][f].tobytes() == got[sa.DEV_DIRECT][f].tobytes(), f
    res = got[sa.DEV_DIRECT]
    # the restatement over the first reads, as a user running the script over their files would, and the bytes of those TSVs
    n_cpu = min(a.cpu_reads, a.reads)
    n_cpu_records = int(first[n_cpu])
    x, y, p = (rows[f][:n_cpu_records].tolist() for f in ("x", "y", "prob_e7"))
    events = [m[:, 1].tolist() for m in paths[:n_cpu]]
    t0 = time.perf_counter()
    exp = ref.deviation(djobs[:n_cpu], first[:n_cpu + 1], x, y, p, mea=events)
    cpu_s = time.perf_counter() - t0
    for f in ("n_aligned", "n_flagged", "n_on_mea", "sum_abs", "max_abs", "max_event", "n_sets"):
        assert res["reads"][f][:n_cpu].tolist() == [r[f] for r in exp["reads"]], f
    tsv_bytes = n_lines = 0
    for j in range(n_cpu):
        r = rows[first[j]:first[j + 1]][:2000]
        ev = np.asarray(reads[j]["events4"], dtype=np.float64).reshape(-1, 4)
        for xi, yi, pe7 in zip(r["x"].tolist(), r["y"].tolist(), r["prob_e7"].tolist()):
            kmer = reads[j]["ref"][xi:xi + K]
            tsv_bytes += len("contig\t%d\t%s\tread_%d\tt\t%d\t%f\t%f\t%f\t%s\t%f\t%f\t%f\t%f\t%f\t%s\n" % (
                xi, kmer, j, yi, ev[yi][0], ev[yi][1], ev[yi][2], kmer, ev[yi][0], ev[yi][1], pe7 / 1e7, ev[yi][0], ev[yi][0], kmer))
        n_lines += len(r)
    n_anchors, n_path = sum(len(j["ax"]) for j in djobs), sum(len(m) for m in paths)
    up = 24 * len(djobs) + 8 * len(djobs) + 8 * n_anchors + 4 * n_path
    down = 8 + res["reads"].nbytes + res["sets"].nbytes + res["hist"].nbytes + res["total_hist"].nbytes
    out = dict(reads=a.reads, events=a.events, records=n_records, total_events=int(sum(j["n_events"] for j in djobs)), anchors=n_anchors,
               path_pairs=n_path, aligned=int(res["reads"]["n_aligned"].sum()), flagged=int(res["reads"]["n_flagged"].sum()),
               sets=int(len(res["sets"])), batch_device_ms=round(st.ms_total_device, 2), mea_kernel_ms=round(mea_info["kernel_ms"], 3),
               deviation_window_ms=[round(v, 3) for v in ms[sa.DEV_WINDOW][1:]],
               deviation_direct_ms=[round(v, 3) for v in ms[sa.DEV_DIRECT][1:]],
               window_over_direct=round(min(ms[sa.DEV_WINDOW][1:]) / min(ms[sa.DEV_DIRECT][1:]), 4),
               pcie_bytes=dict(up=up, down=down, full_tsv_estimate=int(tsv_bytes / max(n_lines, 1) * n_records)),
               cpu_restatement_s=dict(records=n_cpu_records, seconds=round(cpu_s, 3),
                                      extrapolated_to_all_records=round(cpu_s * n_records / max(n_cpu_records, 1), 1)),
               note="one run on one machine")
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
