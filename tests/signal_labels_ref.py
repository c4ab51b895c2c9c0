"""The labelled signal of one read, restated in plain Python / numpy from the definitions in include/signalalign_hip.h (the section on
sa_batch_signal_labels): the MEA set, the full set, the bands, the per-sample map and the per-read record.  Shared by the host and GPU
tests and by probes/signal_labels_rate.py; nothing here calls the library."""
import numpy as np

SEGMENT_FIELDS = ("raw_start", "raw_length", "reference_index", "x", "y", "kmer_id", "prob_units")
BAND_FIELDS = ("raw_start", "raw_length", "reference_index", "x", "n_records")
READ_FIELDS = ("status", "minus_strand", "n_mea", "n_full", "n_bands", "n_samples", "mea_without_record", "n_positions",
               "skipped_positions", "stay_events", "labelled_samples", "first_sample", "end_sample")
NO_RECORDS, NO_PATH = 1, 2


def printed_units(prob_e7):
    """"%f" of prob_e7 / 1e7 in units of 1e-6, through Python's own formatting"""
    return int(("%f" % (int(prob_e7) / 1e7)).replace(".", ""))


def reference_index(job, x):
    return int(job.get("ref_first", 0)) + int(job.get("ref_step", 1)) * int(x) + int(job.get("base_shift", 0))


def segment(job, x, y, kmer_id, prob_e7):
    return (int(job["raw_start"][y]), int(job["raw_length"][y]), reference_index(job, x), int(x), int(y), int(kmer_id),
            printed_units(prob_e7))


def mea_set(job, x, y, kmer_id, prob_e7, path):
    """(segments, path pairs without a record): per pair of the path the record of its cell with the lowest prob_e7, the earliest
    among equals"""
    cells = {}
    for i in range(len(x)):
        c = (int(x[i]), int(y[i]))
        if c not in cells or int(prob_e7[i]) < int(prob_e7[cells[c]]):
            cells[c] = i
    out, missing = [], 0
    for px, py in (path if path is not None else []):
        i = cells.get((int(px), int(py)))
        if i is None:
            missing += 1
        else:
            out.append(segment(job, x[i], y[i], kmer_id[i], prob_e7[i]))
    return out, missing


def full_set(job, x, y, kmer_id, prob_e7):
    """one segment per record, by event; records of one event keep their order"""
    order = sorted(range(len(x)), key=lambda i: int(y[i]))          # (sorted() is stable)
    return [segment(job, x[i], y[i], kmer_id[i], prob_e7[i]) for i in order]


def bands(job, x, y):
    by_x = {}
    for i in range(len(x)):
        by_x.setdefault(int(x[i]), []).append(int(y[i]))
    out = []
    for px in sorted(by_x):
        lo, hi = min(by_x[px]), max(by_x[px])
        start = int(job["raw_start"][lo])
        out.append((start, int(job["raw_start"][hi]) - start + int(job["raw_length"][hi]), reference_index(job, px), px, len(by_x[px])))
    return out


def sample_map(n_samples, segments):
    """per sample the index of the MEA segment that covers it, -1 for none: a segment reaches to the start of the next one, the last
    one to its own end"""
    out = np.full(int(n_samples), -1, dtype=np.int32)
    for i, s in enumerate(segments):
        end = segments[i + 1][0] if i + 1 < len(segments) else s[0] + s[1]
        out[s[0]:end] = i
    return out


def read_record(job, n_records, path, segments, n_missing, n_bands, use_path=True):
    n = len(segments)
    dx = [segments[i][3] - segments[i - 1][3] for i in range(1, n)]
    n_path = len(path) if (use_path and path is not None) else 0
    r = dict(status=NO_RECORDS if n_records == 0 else (NO_PATH if use_path and n_path == 0 else 0),
             minus_strand=int(n > 0 and segments[0][2] >= segments[-1][2]), n_mea=n, n_full=n_records, n_bands=n_bands,
             n_samples=int(job["n_samples"]), mea_without_record=n_missing,
             n_positions=(1 + sum(1 for d in dx if d != 0)) if n else 0, skipped_positions=sum(max(abs(d) - 1, 0) for d in dx),
             stay_events=sum(1 for d in dx if d == 0), labelled_samples=0, first_sample=0, end_sample=0)
    if n:
        r["first_sample"], r["end_sample"] = segments[0][0], segments[-1][0] + segments[-1][1]
        r["labelled_samples"] = r["end_sample"] - r["first_sample"]
    return r


def labels(job, x, y, kmer_id, prob_e7, path, want_mea=True, want_bands=True):
    """all four sets and the per-read record of one job; the sets are lists of tuples in SEGMENT_FIELDS / BAND_FIELDS order"""
    mea, missing = mea_set(job, x, y, kmer_id, prob_e7, path) if want_mea else ([], 0)
    b = bands(job, x, y) if want_bands else []
    return dict(mea=mea, full=full_set(job, x, y, kmer_id, prob_e7), bands=b, samples=sample_map(job["n_samples"], mea),
                read=read_record(job, len(x), path, mea, missing if want_mea else 0, len(b), use_path=want_mea))


def as_tuples(records, fields):
    """a numpy record array of the library as the list of tuples this module makes"""
    return [tuple(int(r[f]) for f in fields) for r in records]


def label_lines(segments, kmer_of):
    """the lines of <label>.labels.tsv / .full.tsv: raw_start raw_length reference_index posterior_probability kmer"""
    return ["%d\t%d\t%d\t%d.%06d\t%s\n" % (s[0], s[1], s[2], s[6] // 1000000, s[6] % 1000000, kmer_of(s[5])) for s in segments]
