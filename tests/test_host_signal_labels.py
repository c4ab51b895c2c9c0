"""Labelled signal without a device: the restatement (signal_labels_ref.py) against a table worked by hand, every answer written out;
the new names in the header, the export list and the ctypes table; every argument check of sa_signal_labels_records answering before
a device is looked for; signalMachine's refusals around --signal-labels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi

import abi_header as hdr
import signal_labels_ref as ref
from test_host_cli_refusals import ONE, SNP, T, TWO_D, USAGE_LINES, collapse_usage, files, run_case, usage   # noqa: F401 (fixtures)

# ---- the hand-worked table: 12 events, 20 records ---------------------------------------------------------------------------------
# events 0 .. 11: 8 samples before the first, 10 unmapped samples between events 6 and 7, 5 samples after the last
RAW_LENGTH = [5, 3, 4, 6, 2, 7, 3, 5, 4, 6, 3, 4]
RAW_START = [8, 13, 16, 20, 26, 28, 35, 48, 53, 57, 63, 66]
N_SAMPLES = 75
# the records in sa_batch_pairs order: (x, y, kmer_id, prob_e7).  Event 4 has none; cell (2, 3) holds three, two of them tied for the
# lowest prob_e7; no record lies on x = 5
RECORDS = [(0, 0, 11, 9000000), (1, 1, 12, 6000004), (1, 2, 12, 2000000), (2, 2, 13, 7000000), (2, 3, 13, 500000), (2, 3, 14, 300000),
           (2, 3, 15, 300000), (3, 3, 16, 100000), (3, 5, 16, 8000000), (4, 5, 17, 1500000), (4, 6, 17, 9999996), (6, 7, 19, 4000000),
           (6, 8, 19, 3000000), (7, 8, 20, 5000000), (7, 9, 20, 10000000), (8, 10, 21, 123456), (8, 11, 21, 0), (9, 11, 22, 2500000),
           (0, 1, 11, 1000000), (7, 10, 20, 800000)]
UNITS = [900000, 600000, 200000, 700000, 50000, 30000, 30000, 10000, 800000, 150000, 1000000, 400000, 300000, 500000, 1000000, 12346, 0,
         250000, 100000, 80000]                                    # "%f" of prob_e7 / 1e7 in units of 1e-6, per record
PATH = [(0, 0), (1, 1), (1, 2), (2, 3), (2, 4), (3, 5), (4, 6), (6, 7), (6, 8), (7, 9), (8, 10), (9, 11)]   # (2, 4): a cell without a record
# the answers, with reference_index written as x (the two jobs below map it differently)
MEA = [(8, 5, 0, 0, 0, 11, 900000), (13, 3, 1, 1, 1, 12, 600000), (16, 4, 1, 1, 2, 12, 200000), (20, 6, 2, 2, 3, 14, 30000),
       (28, 7, 3, 3, 5, 16, 800000), (35, 3, 4, 4, 6, 17, 1000000), (48, 5, 6, 6, 7, 19, 400000), (53, 4, 6, 6, 8, 19, 300000),
       (57, 6, 7, 7, 9, 20, 1000000), (63, 3, 8, 8, 10, 21, 12346), (66, 4, 9, 9, 11, 22, 250000)]
FULL_ORDER = [0, 1, 18, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 19, 16, 17]
BANDS = [(8, 8, 0, 0, 2), (13, 7, 1, 1, 2), (16, 10, 2, 2, 4), (20, 15, 3, 3, 2), (28, 10, 4, 4, 2), (48, 9, 6, 6, 2), (53, 13, 7, 7, 3),
         (63, 7, 8, 8, 2), (66, 4, 9, 9, 1)]
SAMPLES = [-1] * 8 + [0] * 5 + [1] * 3 + [2] * 4 + [3] * 8 + [4] * 7 + [5] * 13 + [6] * 5 + [7] * 4 + [8] * 6 + [9] * 3 + [10] * 4 + [-1] * 5
READ = dict(status=0, n_mea=11, n_full=20, n_bands=9, n_samples=75, mea_without_record=1, n_positions=9, skipped_positions=1, stay_events=2,
            labelled_samples=62, first_sample=8, end_sample=70)
PLUS = dict(ref_first=1000, ref_step=1, base_shift=2)              # reference_index = 1002 + x
MINUS = dict(ref_first=5000, ref_step=-1, base_shift=3)            # reference_index = 5003 - x


def _job(strand):
    return dict(raw_start=np.array(RAW_START), raw_length=np.array(RAW_LENGTH), n_events=12, n_samples=N_SAMPLES, **strand)


def _columns():
    return tuple(np.array([r[i] for r in RECORDS]) for i in range(4))


@pytest.mark.parametrize("strand, index_of, minus", [(PLUS, lambda x: 1002 + x, 0), (MINUS, lambda x: 5003 - x, 1)])
def test_restatement_gives_the_hand_worked_answers(strand, index_of, minus):
    assert len(RECORDS) == 20 and len(SAMPLES) == N_SAMPLES and sorted(FULL_ORDER) == list(range(20))
    mapped = lambda rows: [r[:2] + (index_of(r[2]),) + r[3:] for r in rows]
    got = ref.labels(_job(strand), *_columns(), np.array(PATH))
    assert got["mea"] == mapped(MEA)
    assert got["full"] == [(RAW_START[y], RAW_LENGTH[y], index_of(x), x, y, kmer, UNITS[i]) for i in FULL_ORDER for x, y, kmer, _ in [RECORDS[i]]]
    assert got["bands"] == mapped(BANDS)
    assert got["samples"].tolist() == SAMPLES
    assert got["read"] == dict(READ, minus_strand=minus)
    assert [ref.printed_units(r[3]) for r in RECORDS] == UNITS
    # without a path, and without records
    none = ref.labels(_job(strand), *_columns(), None)
    assert none["mea"] == [] and none["read"]["status"] == ref.NO_PATH and none["full"] == got["full"] and (none["samples"] == -1).all()
    empty = ref.labels(_job(strand), [], [], [], [], np.array(PATH))
    assert empty["read"]["status"] == ref.NO_RECORDS and empty["read"]["mea_without_record"] == 12 and empty["bands"] == []
    # the lines of the label files
    assert ref.label_lines(got["mea"][3:4], lambda k: "K%d" % k) == ["20\t6\t%d\t0.030000\tK14\n" % index_of(2)]


# ---- the names ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_ctypes_agree_on_the_new_names():
    text = hdr.header_text()
    protos = hdr.prototypes(text)
    calls = ["sa_batch_signal_labels", "sa_signal_labels_records", "sa_signal_labels_release", "sa_signal_labels_last_kernel_ms"]
    for name in calls:
        assert name in protos and name in _capi.EXPORTS and name in _capi.SIGNATURES, name
        assert hdr.signature_kinds(*_capi.SIGNATURES[name]) == protos[name], name
        assert hasattr(sa.lib(), name)
    assert len(protos["sa_batch_signal_labels"][1]) == 12 and len(protos["sa_signal_labels_records"][1]) == 17
    for c_name in ("sa_label_job_t", "sa_label_segment_t", "sa_label_band_t", "sa_label_read_t"):
        assert c_name in hdr.struct_names(text) and c_name in _capi.ABI, c_name
    assert _capi.ABI["sa_label_job_t"] is sa.LabelJob
    assert (sa.LABEL_SEGMENT_DTYPE.itemsize, sa.LABEL_BAND_DTYPE.itemsize, sa.LABEL_READ_DTYPE.itemsize) == (40, 32, 128)
    defines = dict(re.findall(r"#define\s+(SA_LABEL_\w+)\s+(\d+)u?\b", text))
    for name, value in (("NO_RECORDS", sa.LABEL_NO_RECORDS), ("NO_PATH", sa.LABEL_NO_PATH), ("MEA", sa.LABEL_MEA), ("FULL", sa.LABEL_FULL),
                        ("BANDS", sa.LABEL_BANDS), ("SAMPLES", sa.LABEL_SAMPLES), ("TIMES", sa.LABEL_TIMES),
                        ("SAMPLE_TILE", sa.LABEL_SAMPLE_TILE), ("N_KERNELS", len(sa.LABEL_KERNELS))):
        assert int(defines["SA_LABEL_" + name]) == value, name
    assert [int(defines["SA_LABEL_K_" + k.upper()]) for k in sa.LABEL_KERNELS] == list(range(len(sa.LABEL_KERNELS)))
    assert (ref.NO_RECORDS, ref.NO_PATH) == (sa.LABEL_NO_RECORDS, sa.LABEL_NO_PATH)


# ---- the argument checks -------------------------------------------------------------------------------------------------------------
ALL = 1 | 2 | 4 | 8


def _code(job=None, records=None, path=PATH, flags=ALL, first=None, n_mea=None):
    """the return code of sa_signal_labels_records for one job, called through ctypes with every array this test's own"""
    job = dict(_job(PLUS), **(job or {}))
    rs = None if job["raw_start"] is None else np.ascontiguousarray(job["raw_start"], dtype=np.int64)
    rl = None if job["raw_length"] is None else np.ascontiguousarray(job["raw_length"], dtype=np.int64)
    p64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))
    p32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    arr = (sa.LabelJob * 1)(sa.LabelJob(p64(rs), p64(rl), job["n_events"], job["n_samples"], job["ref_first"], job["ref_step"], job["base_shift"]))
    cols = [None if c is None else np.ascontiguousarray(c, dtype=dt)
            for c, dt in zip(records if records is not None else _columns(), (np.int32, np.int32, np.int32, np.int64))]
    n = max(len(c) for c in cols if c is not None)
    first = np.array(first if first is not None else [0, n], dtype=np.int64)
    pth = np.ascontiguousarray(path, dtype=np.int32).reshape(-1, 2) if path is not None else None
    paths = (C.c_void_p * 1)(pth.ctypes.data if pth is not None and len(pth) else None)
    cnt = np.array([n_mea if n_mea is not None else (len(pth) if pth is not None else 0)], dtype=np.int64)
    reads = np.zeros(1, dtype=sa.LABEL_READ_DTYPE)
    outs = [C.c_void_p() for _ in range(4)]
    rc = sa.lib().sa_signal_labels_records(arr, 1, p64(first), p32(cols[0]), p32(cols[1]), p32(cols[2]), p64(cols[3]),
                                           paths if path is not None else None, p64(cnt) if path is not None else None, 0, flags,
                                           reads.ctypes.data, *[C.byref(o) for o in outs], None)
    for o in outs:
        sa.lib().sa_free(o)
    return rc


def _with(i, value, column):
    cols = [c.copy() for c in _columns()]
    cols[column][i] = value
    return cols


def test_every_argument_check_answers_before_a_device_is_looked_for():
    assert _code() in (0, -3)                                                  # the table itself passes: SA_OK, or SA_ENODEVICE without a GPU
    assert _code(path=None) in (0, -3) and _code(flags=2) in (0, -3)
    bad = {
        "raw_start NULL": dict(job=dict(raw_start=None)),
        "raw_length NULL": dict(job=dict(raw_length=None)),
        "x NULL": dict(records=(None,) + _columns()[1:]),
        "kmer_id NULL": dict(records=_columns()[:2] + (None,) + _columns()[3:]),
        "a path NULL with pairs": dict(path=np.zeros((0, 2)), n_mea=3),
        "n_events negative": dict(job=dict(n_events=-1)),
        "n_events beyond 2^28": dict(job=dict(n_events=(1 << 28) + 1)),
        "raw_start negative": dict(job=dict(raw_start=[-1] + RAW_START[1:])),
        "raw_start not increasing": dict(job=dict(raw_start=RAW_START[:4] + [20] + RAW_START[5:])),
        "raw_start decreasing": dict(job=dict(raw_start=RAW_START[:4] + [19] + RAW_START[5:])),
        "raw_length zero": dict(job=dict(raw_length=RAW_LENGTH[:3] + [0] + RAW_LENGTH[4:])),
        "an event past the samples": dict(job=dict(n_samples=69)),
        "ref_step zero": dict(job=dict(ref_step=0)),
        "ref_step two": dict(job=dict(ref_step=2)),
        "an MEA event outside the job": dict(path=PATH[:-1] + [(9, 12)]),
        "an MEA event negative": dict(path=[(0, -1)] + PATH),
        "an MEA x negative": dict(path=[(-1, 0)] + PATH[1:]),
        "an MEA x beyond 2^28": dict(path=PATH[:-1] + [(1 << 28, 11)]),
        "MEA events not increasing": dict(path=PATH[:3] + [(1, 2)] + PATH[3:]),
        "a record's y outside the job": dict(records=_with(7, 12, 1)),
        "a record's y negative": dict(records=_with(7, -1, 1)),
        "a record's x negative": dict(records=_with(7, -1, 0)),
        "a record's x beyond 2^28": dict(records=_with(7, 1 << 28, 0)),
        "prob_e7 negative": dict(records=_with(7, -1, 3)),
        "prob_e7 above 1e7": dict(records=_with(7, 10 ** 7 + 1, 3)),
        "samples without the MEA set": dict(flags=8),
        "an unknown flag": dict(flags=1 | 64),
        "first does not start at 0": dict(first=[1, 20]),
        "first decreases": dict(first=[0, -1]),
    }
    got = {what: _code(**kw) for what, kw in bad.items()}
    assert got == {what: -1 for what in bad}
    assert _code(job=dict(n_samples=1 << 31, raw_length=RAW_LENGTH[:-1] + [(1 << 31) - 66])) == -8     # SA_EUNSUPPORTED: 2^31 samples


# ---- signalMachine's refusals ---------------------------------------------------------------------------------------------------------
RAW_ONE = T + ["-q", "{raw}", "-f", "none.fa", "--guide-locate"]
LABELS = ["--signal-labels", "{tmp}/lab"]
REFUSALS = {
    "npread": (ONE + LABELS, "signalMachine: --signal-labels needs a read given as raw current: an .npRead has no raw starts"),
    "two_d": (ONE + LABELS + TWO_D, "signalMachine: --signal-labels does not take --twoD runs"),
    "expectations": (ONE + LABELS + ["-t", "{tmp}/t.expectations"], "signalMachine: --signal-labels needs the alignment mode, not -t/-c"),
    "snp_step": (ONE + LABELS + SNP, "signalMachine: --signal-labels cannot be combined with --snp-step / --snp-sites"),
    "snp_sites": (ONE + LABELS + ["--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv"],
                  "signalMachine: --signal-labels cannot be combined with --snp-step / --snp-sites"),
    "full_alone": (ONE + ["--signal-labels-full"], "signalMachine: --signal-labels-* need --signal-labels <dir>"),
    "bands_alone": (ONE + ["--signal-labels-bands"], "signalMachine: --signal-labels-* need --signal-labels <dir>"),
    "samples_alone": (ONE + ["--signal-labels-samples"], "signalMachine: --signal-labels-* need --signal-labels <dir>"),
    "kmer_index_alone": (ONE + ["--signal-labels-kmer-index", "1"], "signalMachine: --signal-labels-* need --signal-labels <dir>"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_cli_refusal_with_the_usage_text(name, files, usage):
    args, message = REFUSALS[name]
    status, stdout, stderr = run_case(args, files)
    assert status == 1 and stdout == ""
    assert collapse_usage(stderr, usage) == "{usage}\n" + message + "\n" and len(stderr.splitlines()) == USAGE_LINES
    assert os.listdir(files["tmp"]) == [], "a refused command line left a file behind"


@pytest.mark.parametrize("index", ["5", "-1", "9"])
def test_cli_refuses_a_kmer_index_outside_the_models_k(index, files):
    status, stdout, stderr = run_case(RAW_ONE + LABELS + ["--signal-labels-kmer-index", index], files)      # (the bundled model has 5-mers)
    assert status == 1 and stderr.splitlines()[-1] == "signalMachine: --signal-labels-kmer-index takes an index inside the model's k-mer: 0 <= n < 5"
    assert os.listdir(files["tmp"]) == []
