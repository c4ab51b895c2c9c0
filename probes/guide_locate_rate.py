"""Rate of sa_guide_locate_batch: a seeded random reference of 4.6 million bases in 3 contigs with the bundled 6817-base E. coli
window planted in it, and 2000 mutated copies of the bundled 6542-base read (2 % substitutions, 1 % short indels on top of the
read's own errors), half of them reverse-complemented, located in one call.  Medians of 3 calls after a warm-up: the HIP-event
kernel time, the time of the whole call (upload image, kernel, copy back), reads per second over the whole call; beside them the
index's build time on the host (upload included) and its bytes, and the share of reads that come back with status 0 at the
planted locus (right contig and strand, read base 0 within 200 of where the unmutated read's lies).  For scale, what it replaces:
sa_guide_seed over the whole contig on one CPU thread and the numpy restatement (tests/locate_ref.py), seconds per read over 8
reads each.  Writes profiles/guide_locate.json."""
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
import locate_ref as loc  # noqa: E402
from guide_align_rate import mutated  # noqa: E402

CONTIGS = (2500000, 1500000, 600000)
PLANT = (1, 700000)           # contig, offset of the window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_locate.json"))
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--cpu-reads", type=int, default=8)
    a = ap.parse_args()
    if sa.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    read, window = ref.ecoli_pair()
    rng = np.random.default_rng(4600)
    seqs = ["".join(np.array(list("ACGT"))[rng.integers(4, size=n)]) for n in CONTIGS]
    c, at = PLANT
    seqs[c] = seqs[c][:at] + window + seqs[c][at + len(window):]
    names = ["ctg%d" % i for i in range(len(seqs))]
    reads, reverse = [], []
    for k in range(a.reads):
        m = mutated(rng, read)
        reverse.append(k % 2)
        reads.append(ref.reverse_complement(m) if k % 2 else m)
    index = sa.ref_index_build(names, seqs, device=0)
    info = sa.ref_index_info(index)
    kernel, call, res = [], [], None
    for _ in range(4):
        st = {}
        res = sa.guide_locate_batch(index, reads, stats=st)
        kernel.append(st["kernel_ms"])
        call.append(st["call_ms"])
    kernel_ms, call_ms = float(np.median(kernel[1:])), float(np.median(call[1:]))
    # where the unmutated read's first and last base lie, by its guide alignment to the window (the restatement's, at band 128)
    al = ref.banded_cached(read, window, 0, 128)
    first, last = at + al["ref_start"] - al["read_start"], at + al["ref_end"] - 1 + (len(read) - al["read_end"])
    good = 0
    for r, rev in zip(res, reverse):
        want = last if rev else first
        good += r["status"] == 0 and r["contig"] == c and r["reverse"] == rev and abs(r["pos"] - want) <= 200
    case = dict(reads=a.reads, reference_bases=sum(CONTIGS), contigs=len(CONTIGS), kernel_ms=round(kernel_ms, 3), call_ms=round(call_ms, 3),
                reads_per_s=round(a.reads / (call_ms * 1e-3), 1), index_build_s=round(info["build_seconds"], 3),
                index_entries=info["n_entries"], index_table_bits=info["q"], index_device_bytes=info["device_bytes"],
                index_host_bytes=info["host_bytes"], status_0_at_locus=int(good), share_at_locus=round(good / a.reads, 4),
                ambiguous=sum(bool(r["status"] & sa.LOCATE_AMBIGUOUS) for r in res),
                overflow=sum(bool(r["status"] & sa.LOCATE_OVERFLOW) for r in res), min_votes=min(r["votes"] for r in res),
                max_hits=max(r["hits"] for r in res))
    if a.cpu_reads:
        n = a.cpu_reads
        t0 = time.perf_counter()
        seeded = [sa.guide_seed(reads[k], seqs[c], True) for k in range(n)]
        case.update(cpu_guide_seed_s_per_read=round((time.perf_counter() - t0) / n, 3), cpu_reads=n,
                    cpu_guide_seed_found=sum(s["found"] and s["reverse"] == bool(reverse[k]) for k, s in enumerate(seeded)))
        t0 = time.perf_counter()
        restated = loc.build_index(seqs)
        t1 = time.perf_counter()
        same = all(loc.locate(restated, reads[k]) == res[k] for k in range(n))
        case.update(cpu_numpy_index_s=round(t1 - t0, 2), cpu_numpy_s_per_read=round((time.perf_counter() - t1) / n, 4),
                    same_as_restatement=bool(same))
    print(json.dumps(case), flush=True)
    sa.locate_release()
    index.close()
    meta = dict(what="sa_guide_locate_batch: mutated copies of the bundled E. coli 1-D read located in a 4.6 Mbase random reference "
                     "that holds the read's window, one MI355X, one visit",
                made_by=["python probes/guide_locate_rate.py"],
                note="kernel_ms: HIP events around the kernel; call_ms: the whole C call; both the median of 3 calls after a warm-up; "
                     "index_build_s: host build and upload, once; cpu_guide_seed_s_per_read: sa_guide_seed over the planted contig "
                     "(1.5 Mbases, both strands) on one thread; cpu_numpy_s_per_read: tests/locate_ref.py with its index already built")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(_meta=meta, rate=[case]), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
