"""Rate of sa_guide_align_batch: 2000 mutated copies of the bundled E. coli 1-D read (6542 bases; 2 % substitutions, 1 % short
indels on top of the read's own errors) against the read's 6817-base window, one call per band width 64, 128 and 256.  Per band:
the HIP-event kernel time and the time of the whole call (upload image, kernel, copy back, operations unpacked), each the median
of 3 calls after a warm-up; reads per second over the whole call; band steps (anti-diagonals) per second over the kernel time;
the bytes of trace the call writes; and how many reads come back with status 0 and with the unmutated read's score range.
Beside it the numpy restatement (tests/guide_ref.py) on one CPU thread for a few reads: for scale, not a competitor.
Writes profiles/guide_align.json."""
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
import guide_ref as ref  # noqa: E402


def mutated(rng, read):
    out = []
    for c in read:
        u = rng.random()
        if u < 0.02:
            out.append("ACGT"[("ACGT".index(c) + 1 + rng.integers(3)) % 4])
        elif u < 0.025:
            continue
        elif u < 0.03:
            out.append(c)
            out.append("ACGT"[rng.integers(4)])
        else:
            out.append(c)
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_align.json"))
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--cpu-reads", type=int, default=2)
    a = ap.parse_args()
    if sa.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    read, window = ref.ecoli_pair()
    rng = np.random.default_rng(2000)
    jobs = [(mutated(rng, read), window, 0) for _ in range(a.reads)]
    cases = []
    for band in (64, 128, 256):
        prm = sa.guide_params(band=band)
        kernel, call, res = [], [], None
        for _ in range(4):
            st = {}
            res = sa.guide_align_batch(jobs, prm, stats=st)
            kernel.append(st["kernel_ms"])
            call.append(st["call_ms"])
        kernel_ms, call_ms = float(np.median(kernel[1:])), float(np.median(call[1:]))
        steps = sum(len(j[0]) + len(j[1]) for j in jobs)
        row = 64 if band <= 128 else 128
        case = dict(reads=a.reads, band=band, kernel_ms=round(kernel_ms, 2), call_ms=round(call_ms, 2),
                    reads_per_s=round(a.reads / (call_ms * 1e-3), 1), band_steps=steps,
                    band_steps_per_s=round(steps / (kernel_ms * 1e-3)), trace_bytes=sum((len(j[0]) + len(j[1]) + 1) * row for j in jobs),
                    status_0=sum(r["status"] == 0 for r in res), min_score=min(r["score"] for r in res),
                    max_score=max(r["score"] for r in res))
        if a.cpu_reads:
            t0 = time.perf_counter()
            same = True
            for k in range(a.cpu_reads):
                e = ref.banded(jobs[k][0], jobs[k][1], 0, band=band)
                same = same and all(e[f] == res[k][f] for f in ("status", "score", "read_start", "read_end", "ref_start", "ref_end", "ops"))
            case.update(cpu_numpy_s_per_read=round((time.perf_counter() - t0) / a.cpu_reads, 2), cpu_reads=a.cpu_reads,
                        same_as_restatement=bool(same))
        print(json.dumps(case), flush=True)
        cases.append(case)
    sa.guide_release()
    meta = dict(what="sa_guide_align_batch on mutated copies of the bundled E. coli 1-D read, one MI355X, one visit",
                made_by=["python probes/guide_align_rate.py"],
                note="kernel_ms: HIP events around the kernel; call_ms: the whole C call; both the median of 3 calls after a warm-up; "
                     "cpu_numpy_s_per_read: tests/guide_ref.py on one thread, for scale")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(_meta=meta, rate=cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
