"""Labelled signal on the device, on a configs[1]-shaped batch: --reads x --events synthetic reads in one batch, the MEA paths of
sa_batch_mea handed in as the CLI hands them in, and synthetic contiguous event lengths (4 .. 14 samples, mean 9) that give about
45 000 samples per 5000-event read.  Prints one JSON line and writes it to --out:
  kernel_ms              per kernel of sa_batch_signal_labels (SA_LABEL_TIMES: a HIP event pair around each), all four sets asked for
  call_ms                wall time around the C call with and without SA_LABEL_SAMPLES (the per-sample map is 4 bytes per sample
                         over PCIe into pageable memory), and the calls' kernel_ms
  bytes                  what each kernel must move, computed from the shapes
  fill_vs_memset         the per-sample fill next to a hipMemsetAsync of the same byte count, timed with HIP events in this process:
                         the yardstick of a write-only kernel, and the ratio
  cpu_restatement_s      tests/signal_labels_ref.py over the first --cpu-reads reads, one thread, and the same EXTRAPOLATED to all reads
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
from signalalign_amd import synth  # noqa: E402
import signal_labels_ref as ref  # noqa: E402

ALL = sa.LABEL_MEA | sa.LABEL_FULL | sa.LABEL_BANDS | sa.LABEL_SAMPLES


def memset_ms(n_bytes, repeats):
    """the smallest HIP-event time of hipMemsetAsync over n_bytes of device memory, after a warm-up"""
    hip = C.CDLL("libamdhip64.so")

    def chk(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)
    ptr, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    chk(hip.hipMalloc(C.byref(ptr), C.c_size_t(n_bytes)))
    chk(hip.hipEventCreate(C.byref(e0)))
    chk(hip.hipEventCreate(C.byref(e1)))
    times = []
    for _ in range(repeats + 1):
        chk(hip.hipEventRecord(e0, None))
        chk(hip.hipMemsetAsync(ptr, 0xff, C.c_size_t(n_bytes), None))
        chk(hip.hipEventRecord(e1, None))
        chk(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        times.append(ms.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    hip.hipFree(ptr)
    return times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-reads", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signal_labels.json"))
    a = ap.parse_args()
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.nucleotide.6mer.template.model")
    pm = sa.Model.load(model)
    reads = synth.make_reads_parallel(dict(kind="gauss", model=model, events=a.events, kw={}), list(range(a.reads)))
    b = sa.Batch(pm, sa.default_params(threshold=0.01, expansion=50, trace_back=100), reads)
    b.run()
    st = b.stats()
    mea_info = {}
    paths = [m[0] for m in b.mea(stats=mea_info)]
    rng = np.random.default_rng(7)
    ljobs = []
    for r in reads:
        n = len(r["events"])
        lengths = rng.integers(4, 15, size=n)
        start = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        ljobs.append(dict(raw_start=start, raw_length=lengths, n_events=n, n_samples=int(start[-1] + lengths[-1]), ref_first=1000, ref_step=1,
                          base_shift=2))
    kernels, calls = [], {ALL: [], ALL & ~sa.LABEL_SAMPLES: []}
    res = None
    for _ in range(a.repeats + 1):
        for flags in calls:
            t0 = time.perf_counter()
            got = sa.batch_signal_labels(b, ljobs, mea=paths, flags=flags | sa.LABEL_TIMES)
            calls[flags].append(((time.perf_counter() - t0) * 1e3, got["kernel_ms"]))
            if flags == ALL:
                kernels.append(sa.signal_labels_last_kernel_ms())
                res = got
    reads_rec = res["reads"]
    n_rec, n_path, n_mea = int(reads_rec["n_full"].sum()), sum(len(m) for m in paths), int(reads_rec["n_mea"].sum())
    n_events, n_samples, n_bands = sum(j["n_events"] for j in ljobs), int(reads_rec["n_samples"].sum()), int(reads_rec["n_bands"].sum())
    rows, first = b.pairs_all()
    n_x = sum(int(rows["x"][first[j]:first[j + 1]].max() - rows["x"][first[j]:first[j + 1]].min()) + 1 for j in range(a.reads) if first[j + 1] > first[j])
    # bytes each kernel must move: records are 16 bytes, segments 40, bands 32; counters 4, offsets 8
    must = dict(count=16 * n_rec + 4 * n_events, scan_events=(4 + 8) * n_events, scatter=16 * n_rec + 8 * n_events + 4 * n_rec,
                order=8 * n_events + 2 * 4 * n_rec, full=(4 + 16 + 16 + 40) * n_rec, find=8 * n_path + (4 + 16) * n_path + 4 * n_path,
                scan_path=(4 + 8) * n_path, band_acc=16 * n_rec + 3 * 4 * n_rec, scan_bands=(4 + 8) * n_x, job_scan=(2 * 8 + 128) * a.reads,
                mea_emit=(4 + 8 + 16 + 16 + 44) * n_mea, band_emit=3 * 4 * n_x + (8 + 32 + 32) * n_bands, reads=40 * n_mea + 2 * 128 * a.reads,
                fill=4 * n_samples + 4 * n_mea)
    best = {k: min(t[k] for t in kernels[1:]) for k in sa.LABEL_KERNELS}
    ms_memset = memset_ms(4 * n_samples, a.repeats)
    # the restatement over the first reads, one thread
    n_cpu = min(a.cpu_reads, a.reads)
    t0 = time.perf_counter()
    for j in range(n_cpu):
        cols = [rows[f][first[j]:first[j + 1]].tolist() for f in ("x", "y", "kmer_id", "prob_e7")]
        exp = ref.labels(ljobs[j], *cols, paths[j].tolist())
        assert ref.as_tuples(res["mea"][j], ref.SEGMENT_FIELDS) == exp["mea"] and np.array_equal(res["samples"][j], exp["samples"])
        assert ref.as_tuples(res["bands"][j], ref.BAND_FIELDS) == exp["bands"] and ref.as_tuples(res["full"][j], ref.SEGMENT_FIELDS) == exp["full"]
    cpu_s = time.perf_counter() - t0
    with_s, without_s = calls[ALL][1:], calls[ALL & ~sa.LABEL_SAMPLES][1:]
    out = dict(reads=a.reads, events=a.events, records=n_rec, total_events=n_events, samples=n_samples, path_pairs=n_path, mea_segments=n_mea,
               bands=n_bands, x_slots=n_x, sample_tile=sa.LABEL_SAMPLE_TILE, batch_device_ms=round(st.ms_total_device, 2),
               mea_kernel_ms=round(mea_info["kernel_ms"], 3),
               kernel_ms={k: [round(t[k], 4) for t in kernels[1:]] for k in sa.LABEL_KERNELS},
               kernel_ms_sum_of_smallest=round(sum(best.values()), 4),
               bytes=must, gb_per_s={k: round(must[k] / best[k] / 1e6, 1) for k in sa.LABEL_KERNELS if best[k] > 0},
               call_ms=dict(with_samples=[round(w, 2) for w, _ in with_s], without_samples=[round(w, 2) for w, _ in without_s],
                            kernel_ms_with_samples=[round(k, 3) for _, k in with_s], kernel_ms_without_samples=[round(k, 3) for _, k in without_s]),
               fill_vs_memset=dict(bytes=4 * n_samples, fill_ms=[round(t["fill"], 4) for t in kernels[1:]], memset_ms=[round(v, 4) for v in ms_memset],
                                   fill_over_memset=round(best["fill"] / min(ms_memset), 3)),
               cpu_restatement_s=dict(reads=n_cpu, seconds=round(cpu_s, 3), extrapolated_to_all_reads=round(cpu_s * a.reads / max(n_cpu, 1), 1)),
               staged_fill="not measured: no staged variant was written",
               note="one run on one machine")
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
