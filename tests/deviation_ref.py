"""Plain-Python restatement of the guide-deviation stage (sa_batch_guide_deviation, sa_guide_deviation_records), written from the
rules in include/signalalign_hip.h.  It mirrors the three parts of the reference's validation script -- the per-event difference
between the best-posterior position and the guide, the histogram of absolute differences, the sets of consecutive large
differences -- in a job's own coordinates, with the three deliberate differences: ties between equal posteriors go to the largest
x, a set still open when the read ends is kept (open_end = 1; drop_open_sets=True drops it as the reference's loop does), and events
are named by y."""
import bisect

NO_GUIDE, NO_RECORDS = 1, 2


def best_positions(x, y, prob_e7):
    """y -> x of the record with the largest prob_e7, among equal ones the largest x"""
    best = {}
    for xi, yi, pi in zip(x, y, prob_e7):
        key = (int(pi), int(xi))
        if yi not in best or key > best[yi]:
            best[int(yi)] = key
    return {yi: key[1] for yi, key in best.items()}


def guide_position(ax, ay, y):
    """the anchor's x where an anchor names event y, else the integer mean of the neighbours' (or the one that exists); ay ascends"""
    i = bisect.bisect_left(ay, y)
    if i < len(ay) and ay[i] == y:
        return int(ax[i])
    if i == 0:
        return int(ax[0])
    if i == len(ay):
        return int(ax[-1])
    return (int(ax[i - 1]) + int(ax[i])) // 2


def event_rows(ax, ay, x, y, prob_e7, mea_events=(), threshold=10):
    """the aligned events in ascending y, as dicts (y, best_x, guide, diff, abs, on_mea, flagged); [] without anchors"""
    if len(ax) == 0:
        return []
    on_path = set(int(e) for e in mea_events)
    rows = []
    for yi, bx in sorted(best_positions(x, y, prob_e7).items()):
        g = guide_position(ax, ay, yi)
        rows.append(dict(y=yi, best_x=bx, guide=g, diff=bx - g, abs=abs(bx - g), on_mea=yi in on_path, flagged=abs(bx - g) > threshold))
    return rows


def histogram(rows, bucket_size=5, n_buckets=64):
    h = [0] * n_buckets
    for r in rows:
        h[min(r["abs"] // bucket_size, n_buckets - 1)] += 1
    return h


def flagged_sets(rows, drop_open_sets=False):
    """maximal runs of consecutive rows (aligned events) that are flagged"""
    sets, run = [], []

    def close(open_end):
        on = [r["abs"] for r in run if r["on_mea"]]
        sets.append(dict(first_event=run[0]["y"], last_event=run[-1]["y"], count=len(run), peak=max(r["abs"] for r in run),
                         mea_peak=max(on) if on else 0, center_event=sum(r["y"] for r in run) // len(run), open_end=open_end))

    for r in rows:
        if r["flagged"]:
            run.append(r)
        elif run:
            close(0)
            run = []
    if run and not drop_open_sets:
        close(1)
    return sets


def read_summary(ax, rows, n_records, sets):
    r = dict(status=0, n_sets=len(sets), n_aligned=len(rows), n_flagged=sum(q["flagged"] for q in rows),
             n_on_mea=sum(q["on_mea"] for q in rows), sum_abs=sum(q["abs"] for q in rows), max_abs=0, max_abs_mea=0, max_event=0)
    if len(ax) == 0:
        r["status"] = NO_GUIDE
    elif n_records == 0:
        r["status"] = NO_RECORDS
    if rows:
        r["max_abs"] = max(q["abs"] for q in rows)
        r["max_event"] = min(q["y"] for q in rows if q["abs"] == r["max_abs"])
        r["max_abs_mea"] = max([q["abs"] for q in rows if q["on_mea"]] + [0])
    return r


def deviation(jobs, first, x, y, prob_e7, mea=None, threshold=10, bucket_size=5, n_buckets=64, drop_open_sets=False):
    """the whole call: jobs are dicts with ax, ay, n_events; mea per job a list of event indices, or None.  Returns a dict with
    reads (summaries, with set_first), sets (all jobs' back to back), hist (per job), total_hist, rows (per job)."""
    out = dict(reads=[], sets=[], hist=[], total_hist=[0] * n_buckets, rows=[])
    for j, job in enumerate(jobs):
        a, e = int(first[j]), int(first[j + 1])
        rows = event_rows(list(job["ax"]), list(job["ay"]), x[a:e], y[a:e], prob_e7[a:e], mea[j] if mea is not None else (), threshold)
        sets = flagged_sets(rows, drop_open_sets)
        h = histogram(rows, bucket_size, n_buckets)
        r = read_summary(job["ax"], rows, e - a, sets)
        r["set_first"] = len(out["sets"])
        out["reads"].append(r)
        out["sets"] += sets
        out["hist"].append(h)
        out["total_hist"] = [p + q for p, q in zip(out["total_hist"], h)]
        out["rows"].append(rows)
    return out
