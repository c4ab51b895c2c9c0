"""Kernel time of sa_kmer_table_add_batch_at (the k-mer table from the rows that cover labelled positions) on the BASELINE configs[1]
batch (R9.4 6-mer Gaussian, 2000 x 5000 events), every read on a stretch of its own of one contig and a positions table of about
2 x 10^5 lines (every --every-th position under the reads, '+'), beside the unfiltered sa_kmer_table_add_batch on the same batch:
of this build and, with --parent-root <a built checkout of the parent commit>, of that build (a child process that imports the
package from there and runs the same batch).  Each measurement is one add into a fresh table; the smallest of --repeats after one
warm-up (HIP events, device work only).  The cover mask's kernel and the counts pass are reported separately.  Prints one JSON line
and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --package-root <dir>: import signalalign_amd from another built checkout (the child process of --parent-root)
PACKAGE_ROOT = sys.argv[sys.argv.index("--package-root") + 1] if "--package-root" in sys.argv[:-1] else ROOT
sys.path.insert(0, os.path.abspath(PACKAGE_ROOT))
import numpy as np  # noqa: E402

import signalalign_amd as sa  # noqa: E402
from signalalign_amd import synth  # noqa: E402

STRIDE = 20000          # contig positions between the starts of two reads


def main():
    # (the read generator spawns worker processes that import this file: everything runs under the __main__ guard)
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--every", type=int, default=30)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--min-prob", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--unfiltered-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_positions.json"))
    a = ap.parse_args()
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")
    jobs = synth.make_reads_parallel(dict(kind="gauss", model=model, events=a.events, kw={}), list(range(a.reads)))
    pm = sa.Model.load(model)
    b = sa.Batch(pm, sa.default_params(threshold=0.01, expansion=50, trace_back=100), jobs, ambig=sa.default_ambig())
    b.run()
    first = np.zeros(len(jobs) + 1, dtype=np.int64)
    n_pairs = int(b.results_view(first)[1][-1])

    plain_ms, kept_plain = [], 0
    for _ in range(a.repeats + 1):
        tab, info = sa.KmerTable(pm, a.n, a.min_prob), {}
        tab.add_batch(b, 0, stats=info)
        plain_ms.append(info["kernel_ms"])
        kept_plain = len(tab.rows(0))
        tab.close()
    out = dict(reads=a.reads, events=a.events, pairs=n_pairs, N=a.n, min_prob=a.min_prob, step_device_ms=round(b.stats().ms_total_device, 2),
               unfiltered=dict(kernel_ms=[round(v, 3) for v in plain_ms[1:]], kept_rows=kept_plain), note="one run on one machine")
    if a.unfiltered_only:
        b.close()
        print(json.dumps(out), flush=True)
        return

    maps = np.zeros(len(jobs), dtype=sa.TRAIN_JOB_MAP_DTYPE)
    maps["x_sign"], maps["x0"] = 1, STRIDE * np.arange(len(jobs))
    sites = np.concatenate([STRIDE * j + np.arange(0, len(job["ref"]), a.every) for j, job in enumerate(jobs)])
    table = np.zeros(len(sites), dtype=sa.TRAIN_SITE_DTYPE)
    table["pos"] = sites
    at_ms, mask_ms, counts_ms, kept_at, offered = [], [], [], 0, 0
    for _ in range(a.repeats + 1):
        tab, info = sa.KmerTable(pm, a.n, a.min_prob), {}
        tab.set_positions(table)
        tab.add_batch_at(b, maps, 0, stats=info)
        at_ms.append(info["kernel_ms"])
        mask_ms.append(info["mask_ms"])
        counts_ms.append(info["counts_ms"])
        kept_at = len(tab.rows(0))
        offered = int(tab.position_counts()[1].sum())
        tab.close()
    out["filtered"] = dict(position_lines=len(table), kernel_ms=[round(v, 3) for v in at_ms[1:]], mask_kernel_ms=[round(v, 4) for v in mask_ms[1:]],
                           counts_pass_ms=[round(v, 4) for v in counts_ms[1:]], kept_rows=kept_at, coverage_count_total=offered)
    b.close()
    if a.parent_root:   # the parent commit's unfiltered add on the same batch, in a process of its own
        argv = [sys.executable, os.path.abspath(__file__), "--unfiltered-only", "--package-root", a.parent_root, "--reads", str(a.reads), "--events", str(a.events), "--n", str(a.n),
                "--min-prob", str(a.min_prob), "--repeats", str(a.repeats)]
        pr = subprocess.run(argv, capture_output=True, text=True, timeout=900)
        if pr.returncode != 0:
            raise SystemExit("the parent library's run failed: " + pr.stderr[-1000:])
        parent = json.loads(pr.stdout.strip().splitlines()[-1])
        assert parent["pairs"] == n_pairs and parent["unfiltered"]["kept_rows"] == kept_plain
        out["unfiltered_parent_commit"] = parent["unfiltered"]
        out["filtered_over_parent_unfiltered"] = round(min(at_ms[1:]) / min(parent["unfiltered"]["kernel_ms"]), 4)
    out["filtered_over_unfiltered"] = round(min(at_ms[1:]) / min(plain_ms[1:]), 4)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
