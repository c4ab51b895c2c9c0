"""Per-position profile on the device, on a configs[1]-shaped batch: --reads x --events synthetic reads in one batch, laid along one
contig at about --depth reads per position, every other one mapped backward.  Prints one JSON line and writes it to --out:
  add_batch_window_ms    sa_position_profile_add_batch with the LDS window (range pre-pass, spans and accumulate kernels)
  add_batch_direct_ms    the same call with SA_PROFILE_DIRECT: every contribution a global 64-bit atomic -- the A/B of the window,
                         in this one process
  batch_device_ms        the batch's own step time, beside them
  finish_ms              sa_position_profile_finish
  pcie_bytes             what crosses PCIe for the profile (the job map up, the sites down) against the bytes of the full TSV the
                         script would have read (estimated from the rows of the first --cpu-reads reads, formatted as the CLI does)
  cpu_restatement_s      tests/profile_ref.py over the first --cpu-reads reads, one thread, and the same EXTRAPOLATED to all records
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
from signalalign_amd import _capi, synth  # noqa: E402
import profile_ref as ref  # noqa: E402

K = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-reads", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_profile.json"))
    a = ap.parse_args()
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")
    pm = sa.Model.load(model)
    alphabet = pm.alphabet()[0]
    reads = synth.make_reads_parallel(dict(kind="gauss", model=model, events=a.events, kw={}), list(range(a.reads)))
    longest = max(len(r["ref"]) for r in reads)
    spacing = max(1, int(np.mean([len(r["ref"]) for r in reads])) // a.depth)
    contig_len = spacing * a.reads + longest
    job_map = []
    for i, r in enumerate(reads):
        lo, same = spacing * i, i % 2 == 0
        job_map.append(dict(contig=0, pos0=lo if same else lo + len(r["ref"]) - 1, pos_sign=1 if same else -1))
    b = sa.Batch(pm, sa.default_params(threshold=0.01, expansion=50, trace_back=100), reads)
    b.run()
    st = b.stats()
    rows, first = b.pairs_all()
    n_records = int(first[-1])
    ms = {0: [], sa.PROFILE_DIRECT: []}
    fin_ms, tables = [], {}
    for _ in range(a.repeats + 1):
        for flags in (0, sa.PROFILE_DIRECT):
            t = sa.PositionProfile(pm, [contig_len])
            info, fin = {}, {}
            t.add_batch(b, job_map, flags=flags, stats=info)
            tables[flags] = t.finish(stats=fin)
            t.close()
            ms[flags].append(info["kernel_ms"])
            fin_ms.append(fin["kernel_ms"])
    sites, seen = tables[0]
    assert sites.tobytes() == tables[sa.PROFILE_DIRECT][0].tobytes() and seen == tables[sa.PROFILE_DIRECT][1]
    # the restatement over the first reads, as a user running the script over their TSVs would, and the bytes of those TSVs
    n_cpu = min(a.cpu_reads, a.reads)
    files, tsv_bytes = [], 0
    for j in range(n_cpu):
        m, r = job_map[j], rows[first[j]:first[j + 1]]
        files.append((ref.rows_of_records("contig", m["pos0"], m["pos_sign"], K, alphabet, r["x"].tolist(), r["kmer_id"].tolist(),
                                          r["prob_e7"].tolist()), m["pos_sign"] > 0))
        ev = np.asarray(reads[j]["events4"], dtype=np.float64).reshape(-1, 4)
        for x, y, pe7 in zip(r["x"].tolist()[:2000], r["y"].tolist()[:2000], r["prob_e7"].tolist()[:2000]):
            kmer = reads[j]["ref"][x:x + K]
            line = "contig\t%d\t%s\tread_%d\tt\t%d\t%f\t%f\t%f\t%s\t%f\t%f\t%f\t%f\t%f\t%s\n" % (
                m["pos0"] + x, kmer, j, y, ev[y][0], ev[y][1], ev[y][2], kmer, ev[y][0], ev[y][1], pe7 / 1e7, ev[y][0], ev[y][0], kmer)
            tsv_bytes += len(line)
    n_lines = sum(min(2000, int(first[j + 1] - first[j])) for j in range(n_cpu))
    t0 = time.perf_counter()
    P = ref.Profile()
    for file_rows, forward in files:
        P.add_file(file_rows, forward)
    P.finish(alphabet, ["contig"])
    cpu_s = time.perf_counter() - t0
    n_cpu_records = int(first[n_cpu])
    out = dict(reads=a.reads, events=a.events, depth=a.depth, records=n_records, contributions=n_records * K, contig_len=contig_len,
               sites=int(len(sites)), read_count=dict(mean=round(float(sites["read_count"].mean()), 2), max=int(sites["read_count"].max())),
               batch_device_ms=round(st.ms_total_device, 2),
               add_batch_window_ms=[round(x, 3) for x in ms[0][1:]],
               add_batch_direct_ms=[round(x, 3) for x in ms[sa.PROFILE_DIRECT][1:]],
               window_over_direct=round(min(ms[0][1:]) / min(ms[sa.PROFILE_DIRECT][1:]), 4),
               finish_ms=[round(x, 3) for x in fin_ms[2:]],
               pcie_bytes=dict(profile=len(job_map) * 16 + int(len(sites)) * _capi.PROFILE_SITE_DTYPE.itemsize,
                               full_tsv_estimate=int(tsv_bytes / max(n_lines, 1) * n_records)),
               cpu_restatement_s=dict(records=n_cpu_records, seconds=round(cpu_s, 3),
                                      extrapolated_to_all_records=round(cpu_s * n_records / max(n_cpu_records, 1), 1)))
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
