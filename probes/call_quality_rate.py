"""Call quality on the device, chained onto a BASELINE configs[2]-shaped batch (CpG model, X -> C/E at every CpG cytosine): --reads x
--events synthetic reads in one SA_FLAG_SITE_CALLS batch, the MEA paths of sa_batch_mea, synthetic contiguous event lengths (4 .. 14
samples, as probes/signal_labels_rate.py makes them) and a positions table over every site.  Prints one JSON line and writes it to
--out:
  kernel_ms              of sa_batch_call_quality in total (the site fold's kernels are in it) and per kernel (band, calls, gaps: HIP
                         event pairs), with the band's LDS window (the default) and with SA_CQ_BAND_DIRECT (every record a global
                         atomic pair), the two alternating in one process; beside sa_call_scores_add_batch and sa_batch_site_calls on the same batch
  bytes                  what crosses PCIe, up and down, with and without the per-call records
  cpu_restatement_s      tests/call_quality_ref.py over the first --cpu-reads reads, one thread, and the same EXTRAPOLATED to all reads
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
import call_quality_ref as ref  # noqa: E402

K = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-reads", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "call_quality.json"))
    a = ap.parse_args()
    # (the read generator spawns worker processes: they run before this process opens the GPU)
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.cpg.6mer.template.model")
    jobs = synth.make_reads_parallel(dict(kind="gauss", model=model, events=a.events, kw={"cpg_ambiguous": True}), list(range(a.reads)))
    pm = sa.Model.load(model)
    b = sa.Batch(pm, sa.default_params(threshold=0.01, expansion=50, trace_back=100), jobs, ambig=sa.default_ambig({"X": "CE"}),
                 flags=sa.FLAG_SITE_CALLS)
    b.run()
    mea_info = {}
    paths = [m[0] for m in b.mea(stats=mea_info)]
    rng = np.random.default_rng(7)
    maps, cq_jobs, truth = [], [], np.zeros(sum(j["ref"].count("X") for j in jobs), dtype=sa.TRUTH_SITE_DTYPE)
    at = 0
    for j, job in enumerate(jobs):                             # every read on a stretch of its own of one contig, mapped '+'
        x0 = 20000 * j
        maps.append(dict(contig=0, x_sign=1, x0=x0, strand=0, mapped_strand=0, true_letter=-1))
        xs = np.flatnonzero(np.frombuffer(job["ref"].encode(), dtype="S1") == b"X") - (K - 1)
        xs = xs[xs >= 0]
        t = truth[at:at + len(xs)]
        t["pos"], t["change_to"] = x0 + xs, np.where(xs % 2 == 0, b"C", b"E")
        at += len(xs)
        lengths = rng.integers(4, 15, size=len(job["events"]))
        cq_jobs.append(dict(ax=job["ax"], ay=job["ay"], raw_length=lengths, raw_start=np.concatenate([[0], np.cumsum(lengths)[:-1]])))
    acc = sa.CallScores("CE", truth=truth[:at], threshold=0.5)
    variants = dict(window=0, direct=sa.CQ_BAND_DIRECT)
    total = {k: [] for k in variants}
    split = {k: [] for k in variants}
    with_calls, ams, sms = [], [], []
    got = {}
    for _ in range(a.repeats + 1):
        for name, flag in variants.items():
            got[name] = sa.batch_call_quality(acc, b, maps, cq_jobs, mea=paths, flags=flag)
            total[name].append(got[name]["kernel_ms"])
            split[name].append(sa.call_quality_last_kernel_ms())
        full = sa.batch_call_quality(acc, b, maps, cq_jobs, mea=paths, flags=sa.CQ_CALLS)
        with_calls.append((full["kernel_ms"], sa.call_quality_last_kernel_ms()))
        st, st2 = {}, {}
        acc.add_batch(b, maps, stats=st)
        calls = b.site_calls(stats=st2)
        ams.append(st["kernel_ms"])
        sms.append(st2["kernel_ms"])
    keys = ("reads", "gaps", "hist", "total_hist")
    assert all(got["direct"][k].tobytes() == got["window"][k].tobytes() == full[k].tobytes() for k in keys if k != "reads")
    r = got["window"]["reads"]
    assert got["direct"]["reads"].tobytes() == r.tobytes() and int(r["n_calls"].sum()) == len(full["calls"])
    rows, first = b.pairs_all()
    n_rec, n_sites, n_calls = len(rows), sum(len(c["x"]) for c in calls), int(r["n_calls"].sum())
    n_events, n_anchors, n_path, n_gaps = sum(len(j["events"]) for j in jobs), sum(len(j["ax"]) for j in jobs), sum(len(p) for p in paths), int(r["n_gaps"].sum())
    n_slots = 2 * 202
    # the restatement over the first reads, one thread
    n_cpu = min(a.cpu_reads, a.reads)
    t0 = time.perf_counter()
    for j in range(n_cpu):
        c = calls[j]
        table = {(0, maps[j]["x0"] + int(x), 0): int(x) % 2 for x in c["x"]}      # the read's part of the positions table
        sl = slice(int(first[j]), int(first[j + 1]))
        read, exp_calls, gaps, hist = ref.call_quality(maps[j], cq_jobs[j], c["x"], c["prob"][:, :2], rows["x"][sl], rows["y"][sl],
                                                       paths[j][:, 1], 0.5, table)
        assert {k: int(r[j][k]) for k in read} == read, j
        assert (got["window"]["hist"][j] == hist).all()
        a0 = int(full["reads"]["call_first"][j])
        assert [int(v) for v in full["calls"]["delta2"][a0:a0 + len(exp_calls)]] == [k["delta2"] for k in exp_calls]
    cpu_s = time.perf_counter() - t0
    best = {k: {q: min(t[q] for t in split[k][1:]) for q in sa.CQ_KERNELS} for k in variants}
    out = dict(reads=a.reads, events=a.events, records=n_rec, sites=n_sites, calls=n_calls, correct=int(r["n_correct"].sum()),
               outside=int(r["n_outside"].sum()), total_events=n_events, anchors=n_anchors, path_pairs=n_path, gaps=n_gaps,
               records_per_site=round(n_rec / max(n_sites, 1), 2), batch_device_ms=round(b.stats().ms_total_device, 2),
               mea_kernel_ms=round(mea_info["kernel_ms"], 3),
               kernel_ms_total={k: [round(v, 3) for v in total[k][1:]] for k in variants},
               kernel_ms_total_with_calls=[round(v, 3) for v, _ in with_calls[1:]],
               kernel_ms_per_kernel={k: {q: [round(t[q], 4) for t in split[k][1:]] for q in sa.CQ_KERNELS} for k in variants},
               kernel_ms_per_kernel_with_calls={q: [round(t[q], 4) for _, t in with_calls[1:]] for q in sa.CQ_KERNELS},
               band_smallest_ms={k: round(best[k]["band"], 4) for k in variants},
               add_batch_kernel_ms=[round(v, 3) for v in ams[1:]], site_calls_kernel_ms=[round(v, 3) for v in sms[1:]],
               bytes=dict(up=8 * n_anchors + 16 * n_events + 4 * n_path + 4 * n_sites + (32 + 40) * a.reads,
                          down=(112 + 8 * n_slots) * a.reads + 8 * n_slots + 16 * n_gaps, down_calls=56 * n_calls),
               cpu_restatement_s=dict(reads=n_cpu, seconds=round(cpu_s, 3), extrapolated_to_all_reads=round(cpu_s * a.reads / max(n_cpu, 1), 1)),
               note="one run on one machine")
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    acc.close()
    b.close()


if __name__ == "__main__":
    main()
