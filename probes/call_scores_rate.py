"""The call scores on the device (sa_sort_u64, sa_call_scores_add_batch, sa_call_scores_finish).  Prints one JSON line and writes it
to --out:
  sort            per input (10^7 and 10^8 random scores, 10^8 six-decimal scores): kernel_ms of sa_sort_u64, the passes that ran (a
                  digit in which all keys agree costs none), keys/s, the bytes per second that passes x 16 B per key imply and their
                  share of --hbm-bytes-per-s; np.sort of the same array on one CPU thread beside it
  add_batch       kernel_ms of sa_call_scores_add_batch chained onto a BASELINE configs[2]-shaped batch (CpG model, X -> C/E at every
                  CpG cytosine) with a positions table over every site, beside sa_batch_site_calls' kernels on the same batch, and the
                  bytes of calls that no longer cross PCIe
  finish          kernel_ms of sa_call_scores_finish with --finish-scores level-0 scores per class and letter, and the restatement's
                  sort and searches (tests/call_scores_ref.py's numpy calls) on one CPU thread at --cpu-scores per class, EXTRAPOLATED
                  linearly to the device's size
Each device time is the smallest of --repeats calls after one warm-up call.  --sections sort runs the sort alone, which starts no
child process: the form to run under `rocprofv3 --kernel-trace --stats` for the per-kernel split of a pass."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import signalalign_amd as sa  # noqa: E402
from signalalign_amd import synth  # noqa: E402

K = 6


def sort_case(name, keys, repeats, hbm):
    ms = []
    for _ in range(repeats + 1):
        st = {}
        got = sa.sort_u64(keys, stats=st)
        ms.append(st["kernel_ms"])
    t0 = time.perf_counter()
    exp = np.sort(keys)
    cpu_s = time.perf_counter() - t0
    assert got.tobytes() == exp.tobytes()
    differ = int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys))        # the bits in which some keys differ
    passes = sum(1 for b in range(8) if (differ >> (8 * b)) & 255)
    best = min(ms[1:])
    implied = passes * 16.0 * len(keys) / (best * 1e-3)
    return dict(input=name, n=len(keys), passes=passes, kernel_ms=[round(v, 3) for v in ms[1:]], keys_per_s=round(len(keys) / (best * 1e-3), 0),
                implied_bytes_per_s=round(implied, 0), share_of_hbm=round(implied / hbm, 4), np_sort_one_thread_s=round(cpu_s, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--big", type=int, default=100000000)
    ap.add_argument("--finish-scores", type=int, default=100000000)
    ap.add_argument("--cpu-scores", type=int, default=10000000)
    ap.add_argument("--hbm-bytes-per-s", type=float, default=8.0e12)
    ap.add_argument("--sections", default="sort,finish,add_batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "call_scores.json"))
    a = ap.parse_args()
    sections = a.sections.split(",")
    # (the read generator spawns worker processes: they run before this process opens the GPU)
    model = os.path.join(ROOT, "tests", "golden", "models", "testModelR9.4_450bps.cpg.6mer.template.model")
    spec = dict(kind="gauss", model=model, events=a.events, kw={"cpg_ambiguous": True})
    jobs = synth.make_reads_parallel(spec, list(range(a.reads))) if "add_batch" in sections else []
    rng = np.random.default_rng(1)
    out = dict(hbm_bytes_per_s=a.hbm_bytes_per_s, sort_tile=sa.SORT_TILE, note="one run on one machine")

    # ---- the sort ----
    big = rng.random(a.big if "sort" in sections else 10)
    out["sort"] = [sort_case("random scores", big[:a.big // 10].view(np.uint64), a.repeats, a.hbm_bytes_per_s),
                   sort_case("random scores", big.view(np.uint64), a.repeats, a.hbm_bytes_per_s),
                   sort_case("six-decimal scores", np.round(big, 6).view(np.uint64), a.repeats, a.hbm_bytes_per_s)]
    del big

    # ---- finish: --finish-scores per class and letter at level 0, template strand ----
    n = a.finish_scores if "finish" in sections else 1000
    acc = sa.CallScores("CE")
    for _ in range(2):                                         # (half of an add's records are positives of a letter)
        p = rng.random(n)
        acc.add_records(0, 0, np.stack([p, 1.0 - p], axis=1), rng.integers(0, 2, n, dtype=np.int8))
    fms = []
    for _ in range(a.repeats + 1):
        st = {}
        rows = acc.finish(stats=st)[0]
        fms.append(st["kernel_ms"])
    acc.close()
    m = a.cpu_scores
    pos, neg = rng.random(m).view(np.uint64), rng.random(m).view(np.uint64)
    t0 = time.perf_counter()
    s_neg, s_pos = np.sort(neg), np.sort(pos)
    lo, hi = np.searchsorted(s_neg, pos, side="left"), np.searchsorted(s_neg, pos, side="right")
    auc2 = int(lo.sum(dtype=np.uint64)) + int(hi.sum(dtype=np.uint64))
    grid = np.array([k / 1000.0 for k in range(1001)]).view(np.uint64)
    ge = (len(s_pos) - np.searchsorted(s_pos, grid, side="left"), len(s_neg) - np.searchsorted(s_neg, grid, side="left"))
    cpu_s = time.perf_counter() - t0
    assert auc2 > 0 and len(ge[0]) == 1001
    out["finish"] = dict(scores_per_class=[int(rows[0]["n_pos"]), int(rows[0]["n_neg"])], letters=2, rows=len(rows),
                         kernel_ms=[round(v, 2) for v in fms[1:]],
                         cpu_restatement_s=dict(scores_per_class=m, letters=1, seconds=round(cpu_s, 2),
                                                extrapolated_to_the_device_size=round(cpu_s * 2.0 * n / m, 1)))

    # ---- add_batch on the configs[2] batch ----
    if "add_batch" not in sections:
        print(json.dumps(out), flush=True)
        return
    pm = sa.Model.load(model)
    b = sa.Batch(pm, sa.default_params(threshold=0.01, expansion=50, trace_back=100), jobs, ambig=sa.default_ambig({"X": "CE"}),
                 flags=sa.FLAG_SITE_CALLS)
    b.run()
    maps, truth = [], np.zeros(sum(j["ref"].count("X") for j in jobs), dtype=sa.TRUTH_SITE_DTYPE)
    at = 0
    for j, job in enumerate(jobs):                             # every read on a stretch of its own of one contig, mapped '+'
        x0 = 20000 * j
        maps.append(dict(contig=0, x_sign=1, x0=x0, strand=0, mapped_strand=0, true_letter=-1))
        xs = np.flatnonzero(np.frombuffer(job["ref"].encode(), dtype="S1") == b"X") - (K - 1)
        xs = xs[xs >= 0]
        t = truth[at:at + len(xs)]
        t["pos"], t["change_to"] = x0 + xs, np.where(xs % 2 == 0, b"C", b"E")
        at += len(xs)
    acc = sa.CallScores("CE", truth=truth[:at])
    ams, sms = [], []
    for _ in range(a.repeats + 1):
        st, st2 = {}, {}
        acc.add_batch(b, maps, stats=st)
        calls = b.site_calls(stats=st2)
        ams.append(st["kernel_ms"])
        sms.append(st2["kernel_ms"])
    rows, _, counts = acc.finish()
    n_calls = sum(len(c["x"]) for c in calls)
    assert int(rows[0]["n_pos"] + rows[0]["n_neg"]) == (a.repeats + 1) * n_calls and counts["unlabelled"] == 0
    out["add_batch"] = dict(reads=a.reads, events=a.events, reported_sites=n_calls, truth_lines=at, batch_device_ms=round(b.stats().ms_total_device, 2),
                            add_batch_kernel_ms=[round(v, 3) for v in ams[1:]], site_calls_kernel_ms=[round(v, 3) for v in sms[1:]],
                            pcie_bytes_not_crossing=n_calls * (4 + 2 * 8 * 2))   # per call: site index, units and prob of two letters
    acc.close()
    b.close()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
