"""Cost of the raw-current front door: sa_npread_from_raw_batch (detection, MoM scalings, event alignment, k_raw_finish, the
host's p_model_state and make_event_map) on 2000 copies of the first 45 000 samples of the read-108 fixture with the matching
prefix of its sequence, against sa_raw_event_align_batch -- the call it is built from -- on the same input, from this tree's
library and, with --parent-lib, from a build of the parent commit (on the same GPU in the same session: each library is
measured in a child process of its own, one after the other).  Per call: the whole-call wall time around the C entry point
(results released outside the timed region) and the HIP-event kernel time, each the smallest of three calls after a warm-up;
for the new call also k_raw_finish alone.  Writes profiles/raw_front_door.json.

    python probes/raw_front_door_rate.py [--parent-lib <libsignalalign_hip.so of the parent commit>]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL = os.path.join(GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
SAMPLES, K = 45000, 5


class RawJob(C.Structure):
    _fields_ = [("raw", C.POINTER(C.c_int16)), ("n_samples", C.c_int64), ("digitisation", C.c_float), ("offset", C.c_float),
                ("range", C.c_float), ("sample_rate", C.c_float), ("start_time", C.c_float)]


class RawNpRead(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_events", C.c_int64), ("events4", C.c_void_p), ("kmer_idx", C.c_void_p),
                ("move", C.c_void_p), ("p_model_state", C.c_void_p), ("raw_start", C.c_void_p), ("raw_length", C.c_void_p),
                ("read_len", C.c_int64), ("strand_event_map", C.c_void_p), ("mom_shift", C.c_double), ("mom_scale", C.c_double)]


RAW_EVENT_BYTES = 64


def workload(L, model):
    """(raw prefix, attributes, sequence prefix): the bases of the prefix come from the read's own base-to-event map"""
    f = np.load(os.path.join(GOLDEN, "raw", "read108_dna.npz"))
    a = np.asarray(f["attrs_f64_bits"], dtype=np.uint64).view(np.float64)
    seq = open(os.path.join(GOLDEN, "npReads", "r9p4_oneD.npRead")).read().split("\n")[2].strip()
    raw = np.ascontiguousarray(f["raw"], dtype=np.int16)
    ev, st, _, _ = old_call(L, model, [raw], a, [seq], keep=True)
    assert st[0] == 0
    ev = ev[0]
    inside = (ev["raw_start"] + ev["raw_length"] <= SAMPLES) & (ev["kmer_idx"] >= 0)
    return raw[:SAMPLES].copy(), a, seq[:int(ev["kmer_idx"][inside].max()) + K]


def job_array(raws, a):
    arr = (RawJob * len(raws))()
    for i, r in enumerate(raws):
        arr[i] = RawJob(r.ctypes.data_as(C.POINTER(C.c_int16)), len(r), a[0], a[1], a[2], a[3], a[4])
    return arr


def old_call(L, model, raws, a, seqs, keep=False):
    n = len(raws)
    arr = job_array(raws, a)
    sp = (C.c_char_p * n)(*[s.encode() for s in seqs])
    ev_p, ev_n = (C.c_void_p * n)(), (C.c_int64 * n)()
    st = (C.c_int32 * n)()
    kms = C.c_double()
    t0 = time.perf_counter()
    rc = L.sa_raw_event_align_batch(model, arr, sp, n, None, 0, 0, ev_p, ev_n, None, None, st, None, None, C.byref(kms))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    dt = np.dtype([("raw_start", "<i8"), ("raw_length", "<i8"), ("mean", "<f8"), ("stdv", "<f8"), ("start", "<f8"),
                   ("length", "<f8"), ("kmer_idx", "<i4"), ("move", "<i4"), ("p_model_state", "<f8")])
    assert dt.itemsize == RAW_EVENT_BYTES
    out = []
    for i in range(n):
        if keep:
            buf = (C.c_char * (RAW_EVENT_BYTES * ev_n[i])).from_address(ev_p[i])
            out.append(np.frombuffer(buf, dtype=dt).copy())
        L.sa_free(ev_p[i])
    return out, list(st), wall, kms.value


def new_call(L, model, raws, a, seqs):
    n = len(raws)
    arr = job_array(raws, a)
    sp = (C.c_char_p * n)(*[s.encode() for s in seqs])
    res = (RawNpRead * n)()
    kms = C.c_double()
    t0 = time.perf_counter()
    rc = L.sa_npread_from_raw_batch(model, arr, sp, n, None, 0, 0, res, C.byref(kms))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    ok, rows = sum(r.status == 0 for r in res), int(res[0].n_events)
    L.sa_raw_npread_free(res, n)
    return wall, kms.value, L.sa_npread_last_finish_ms(), ok, rows


def child(lib_path, reads, with_new):
    L = C.CDLL(lib_path)
    L.sa_model_load.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p]
    L.sa_free.argtypes = [C.c_void_p]
    L.sa_free.restype = None
    L.sa_raw_event_align_batch.argtypes = [C.c_void_p, C.POINTER(RawJob), C.POINTER(C.c_char_p), C.c_int64, C.c_void_p, C.c_int,
                                           C.c_uint, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    if with_new:
        L.sa_npread_from_raw_batch.argtypes = [C.c_void_p, C.POINTER(RawJob), C.POINTER(C.c_char_p), C.c_int64, C.c_void_p, C.c_int,
                                               C.c_uint, C.POINTER(RawNpRead), C.POINTER(C.c_double)]
        L.sa_raw_npread_free.argtypes = [C.POINTER(RawNpRead), C.c_int64]
        L.sa_raw_npread_free.restype = None
        L.sa_npread_last_finish_ms.restype = C.c_double
    if L.sa_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    model = C.c_void_p()
    assert L.sa_model_load(C.byref(model), MODEL.encode(), None) == 0
    raw, a, seq = workload(L, model)
    raws, seqs = [raw] * reads, [seq] * reads
    out = dict(reads=reads, samples_per_read=len(raw), bases_per_read=len(seq))
    old = [old_call(L, model, raws, a, seqs)[2:] for _ in range(4)][1:]
    out.update(raw_event_align_call_ms=round(min(w for w, _ in old), 2), raw_event_align_kernel_ms=round(min(k for _, k in old), 2))
    if with_new:
        new = [new_call(L, model, raws, a, seqs) for _ in range(4)][1:]
        out.update(npread_call_ms=round(min(r[0] for r in new), 2), npread_kernel_ms=round(min(r[1] for r in new), 2),
                   raw_finish_kernel_ms=round(min(r[2] for r in new), 3), reads_status_0=new[0][3], rows_per_read=new[0][4])
        # the calls alternate once more, so that neither is measured only behind the other
        again = min(old_call(L, model, raws, a, seqs)[2] for _ in range(3))
        out.update(raw_event_align_call_ms_after=round(again, 2))
    print(json.dumps(out), flush=True)


def run_child(lib_path, reads, with_new):
    argv = [sys.executable, os.path.abspath(__file__), "--child", lib_path, "--reads", str(reads)] + (["--with-new"] if with_new else [])
    pr = subprocess.run(argv, capture_output=True, text=True, timeout=900)
    if pr.returncode != 0:
        raise SystemExit("measuring %s failed:\n%s" % (lib_path, pr.stderr[-2000:]))
    return json.loads(pr.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_front_door.json"))
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--parent-lib", default=None, help="libsignalalign_hip.so built from the parent commit")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--with-new", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reads, a.with_new)
        return
    here = run_child(os.path.join(ROOT, "signalalign_amd", "lib", "libsignalalign_hip.so"), a.reads, True)
    result = dict(this_tree=here)
    base = here["raw_event_align_call_ms"]
    if a.parent_lib:
        parent = run_child(os.path.abspath(a.parent_lib), a.reads, False)
        result["parent_commit"] = parent
        base = parent["raw_event_align_call_ms"]
    ratio = here["npread_call_ms"] / base
    result.update(baseline="parent commit's sa_raw_event_align_batch" if a.parent_lib else "this tree's sa_raw_event_align_batch",
                  baseline_call_ms=base, npread_call_ms=here["npread_call_ms"], ratio_npread_over_baseline=round(ratio, 3),
                  within_10_percent=bool(ratio <= 1.10))
    print(json.dumps(result), flush=True)
    meta = dict(what="sa_npread_from_raw_batch against sa_raw_event_align_batch, %d copies of read 108's first %d samples, one MI355X, "
                     "one visit" % (a.reads, SAMPLES),
                made_by=["python probes/raw_front_door_rate.py --parent-lib <the parent commit's library>"],
                note="*_call_ms: wall time around the C entry point; *_kernel_ms: HIP events; each the smallest of three calls after a "
                     "warm-up; raw_finish_kernel_ms: k_raw_finish alone; the requirement is ratio_npread_over_baseline <= 1.10")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(_meta=meta, **result), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
