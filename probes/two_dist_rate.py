"""Step time of the two-distribution emission on the kernel families the benchmark times, on a resident batch:

    python probes/two_dist_rate.py [--reads 2000] [--events 5000] [--steps 5] [--label NAME] [--out FILE.jsonl]

Two batches -- configs[2]-shaped CpG reads (every CpG cytosine X -> C / E: the ring kernels, several paths per cell) and 6-mer reads
with the anchors of a real guide alignment (the strip kernels) -- each aligned
  * with SA_EMISSION_TWO_DIST and SA_FLAG_TWO_DIST_ALL_KERNELS (a library without the flag: flags 0, i.e. the fall-back of the whole
    batch to the reference-ordered kernels -- run this file from a checkout of that commit for the comparison), and
  * with SA_EMISSION_MEAN_ONLY, flags 0: the same kernels without the noise term.
One JSON line per run (appended to --out): label, batch, emission, flags, the routing sa_batch_stats reports, the median and the
extremes of the step times (sa_batch_run on the resident batch: kernels, finalisation and the result copy; it returns when the
results are in host memory) and the kernels' own forward / backward milliseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.getcwd() if os.path.isdir(os.path.join(os.getcwd(), "signalalign_amd")) else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import signalalign_amd as sa
from signalalign_amd import synth
import sa_cases as cases

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2000)
ap.add_argument("--events", type=int, default=5000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_dist_kernels.jsonl"))
a = ap.parse_args()

FLAG = getattr(sa, "FLAG_TWO_DIST_ALL_KERNELS", 0)
if sa.device_count() < 1:
    raise SystemExit("two_dist_rate: no HIP device")


def timed(name, model_path, emission, flags, jobs, ambig):
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    m = sa.Model.create(alpha, k, t10, tab)
    m.set_emission(emission)
    p = sa.default_params()
    t0 = time.perf_counter()
    b = sa.Batch(m, p, jobs, ambig=ambig, flags=flags)
    t_create = time.perf_counter() - t0
    b.run()                                            # warm-up: code objects, the pools' first blocks
    steps = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        b.run()
        steps.append((time.perf_counter() - t0) * 1e3)
    st = b.stats()
    n_pairs = sum(b.n_pairs(j) for j in range(0, len(jobs), max(len(jobs) // 50, 1)))
    rec = dict(label=a.label, batch=name, reads=len(jobs), events=a.events, emission=emission, flags=flags,
               regions=st.n_regions, fast=st.n_fast_regions, ring=st.n_ring_regions, strip=st.n_strip_regions, chunks=st.n_chunks,
               step_ms_median=float(np.median(steps)), step_ms_min=min(steps), step_ms_max=max(steps), steps=a.steps,
               ms_forward=st.ms_forward, ms_backward=st.ms_backward, create_ms=t_create * 1e3, pairs_sampled=int(n_pairs))
    b.close()
    m.close()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


cpg = cases.synthetic_jobs(cases.MODEL_CPG, a.reads, a.events, cpg_ambiguous=True)
amb = sa.default_ambig({"X": "CE"})
real = cases.realistic_anchor_jobs(cases.MODEL_6MER, a.reads, a.events)
for name, model_path, jobs, ambig in (("cpg", cases.MODEL_CPG, cpg, amb), ("realistic", cases.MODEL_6MER, real, None)):
    timed(name, model_path, 1, FLAG, jobs, ambig)
    timed(name, model_path, 0, 0, jobs, ambig)
