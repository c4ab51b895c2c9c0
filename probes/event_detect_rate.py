"""Event detection rate (sa_detect_events_batch): HIP-event time of the detection kernels and the whole call on
synthetic raw reads -- 2000 x 45 000 samples (about the raw signal behind bench configs[1]'s 5000-event reads) and
200 x 450 000.  Prints one JSON line per shape.  Usage: event_detect_rate.py [--reps R] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import signalalign_amd as sa          # noqa: E402
from signalalign_amd import synth     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quick", action="store_true", help="one repetition of each shape (for a profiler run)")
a = ap.parse_args()
reps = 1 if a.quick else a.reps
for n_reads, n_samples in ((2000, 45000), (200, 450000)):
    base = [synth.make_raw(70000 + i, n_samples // 9 + 1, n_samples=n_samples) for i in range(min(n_reads, 50))]
    jobs = [base[i % len(base)] for i in range(n_reads)]
    sa.detect_events_batch(jobs[:64])                         # warm-up: module load, workspace
    kms, wall, n_ev = [], [], 0
    for _ in range(reps):
        st = {}
        t0 = time.perf_counter()
        got = sa.detect_events_batch(jobs, stats=st)
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(st["kernel_ms"])
        n_ev = sum(len(g) for g in got)
    k = float(np.median(kms))
    print(json.dumps(dict(reads=n_reads, samples_per_read=n_samples, events=n_ev, kernel_ms_median=round(k, 3),
                          kernel_ms_all=[round(x, 3) for x in kms], call_ms_median=round(float(np.median(wall)), 2),
                          samples_per_s=round(n_reads * n_samples / (k * 1e-3), 0))), flush=True)
