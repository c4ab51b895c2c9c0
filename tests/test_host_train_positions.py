"""The k-mer training table from the rows that cover labelled positions, without a device: the restatement
(tests/train_positions_ref.py) on a table worked out by hand; header, EXPORTS and ctypes agree on the new symbols and structs; the
argument checks that come before any device use; signalMachine's three new refusals and its usage text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import signalalign_amd as sa
from signalalign_amd import _capi

from abi_header import header_text

import kmer_training_ref as kref
import sa_cases as cases
import train_positions_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
MODEL = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
NPREAD = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")

POSITIONS = """# contig position strand change_from change_to
chr1\t10\t+\tC\tE
chr1\t12\t+\tC\tE
chr1\t10\t-\tG\tX
chr1\t2\t+\tC\tE
chr1\t10\t+\tC\tO
chr2\t7\t-\tC\tE
"""
K = 5
#        contig  ref_index strand forward kmer posterior     what the row shows
ROWS = [("chr1", 6, "t", True, 7, "0.900000"),     # 0  p - (k - 1) of 10+: kept
        ("chr1", 5, "t", True, 7, "0.990000"),     # 1  p - k of 10+ (and past 2+): dropped
        ("chr1", 10, "t", True, 7, "0.900000"),    # 2  p of 10+, p - 2 of 12+: kept, counts for both
        ("chr1", 13, "t", True, 7, "0.990000"),    # 3  p + 1 of 12+: dropped
        ("chr1", 8, "t", True, 7, "0.950000"),     # 4  two positions closer than k: counts for 10+ and 12+
        ("chr1", 0, "t", True, 9, "0.700000"),     # 5  p < k - 1: the window of 2+ starts below 0; kept
        ("chr1", 3, "t", True, 9, "0.990000"),     # 6  p + 1 of 2+: dropped
        ("chr1", 9, "c", True, 7, "0.990000"),     # 7  a c row of a forward read pairs with '-': covers 10- only
        ("chr1", 9, "t", False, 7, "0.800000"),    # 8  a backward-mapped read's t row pairs with '-': covers 10-
        ("chr1", 9, "c", False, 7, "0.600000"),    # 9  a backward-mapped read's c row pairs with '+': covers 10+ and 12+
        ("chr3", 10, "t", True, 7, "0.990000"),    # 10 a contig the file does not name: dropped
        ("chr2", 7, "t", True, 7, "0.990000"),     # 11 chr2 has 7 on '-' only: dropped
        ("chr2", 3, "t", False, 11, "0.500000"),   # 12 p - (k - 1) of chr2 7-, posterior == min_prob: kept
        ("chr1", 10, "t", True, 7, "0.400000"),    # 13 below min_prob: not offered, not counted
        ("chr1", 12, "t", True, 7, "0.900000")]    # 14 p of 12+: kept
OFFERED = [0, 2, 4, 5, 7, 8, 9, 12, 14]
COUNTS = {("chr1", 10, "+"): 4, ("chr1", 12, "+"): 4, ("chr1", 10, "-"): 2, ("chr1", 2, "+"): 1, ("chr2", 7, "-"): 1}
# top 2 per (strand, k-mer): t/7 has 0.95 (row 4), then 0.9 three times -> the earliest, row 0; the c rows of k-mer 7 are their own group
KEPT = {("t", 7): [4, 0], ("t", 9): [5], ("t", 11): [12], ("c", 7): [7, 9]}
COVERAGE = "chr1\t2\t+\t1\nchr1\t10\t+\t4\nchr1\t12\t+\t4\nchr1\t10\t-\t2\nchr2\t7\t-\t1\n"


def test_restatement_on_a_hand_worked_table():
    lines = ref.parse_positions(POSITIONS)
    assert len(lines) == 6 and len(set(lines)) == 5                      # the duplicate line is one key
    idx, counts = ref.offered([(r[0], r[1], r[2], r[3], r[5]) for r in ROWS], lines, K, 0.5)
    assert idx == OFFERED
    assert counts == COUNTS
    assert sum(counts.values()) == len(OFFERED) + 3                      # rows 2, 4 and 9 count twice
    kept = kref.top_n([(ROWS[i][2], ROWS[i][4], "0.000000", ROWS[i][5], i) for i in idx], 2, 0.5)
    assert {key: [r[4] for r in v] for key, v in kept.items()} == KEPT
    assert ref.coverage_lines(lines, counts) == COVERAGE
    assert [ref.site_strand(f, s) for f in (True, False) for s in "tc"] == ["+", "-", "-", "+"]


NEW = ("sa_kmer_table_set_positions", "sa_kmer_table_add_batch_at", "sa_kmer_table_position_counts", "sa_kmer_table_add_at_times")
WIDTH = {"int32_t": 4, "int64_t": 8}


def _header_struct(name):
    body = re.search(r"typedef struct \w+ \{([^}]*)\} %s;" % name, header_text()).group(1)
    fields = []
    for typ, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        fields += [(n.strip(), WIDTH[typ]) for n in names.split(",")]
    return fields


def test_header_exports_and_ctypes_agree():
    hdr = header_text()
    L = sa.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _capi.EXPORTS and hasattr(L, name), name
    for cname, struct, dtype, size in (("sa_train_site_t", sa.TrainSite, sa.TRAIN_SITE_DTYPE, 16),
                                       ("sa_train_job_map_t", sa.TrainJobMap, sa.TRAIN_JOB_MAP_DTYPE, 24)):
        fields = _header_struct(cname)
        assert sum(w for _, w in fields) == size == C.sizeof(struct) == dtype.itemsize
        assert [(n, w) for n, w in fields] == [(n, C.sizeof(t)) for n, t in struct._fields_]
        assert [n for n, _ in fields] == list(dtype.names)
        assert [dtype.fields[n][1] for n in dtype.names] == [getattr(struct, n).offset for n in dtype.names]
    for name in ("set_positions", "add_batch_at", "position_counts"):
        assert callable(getattr(sa.KmerTable, name))


def test_argument_checks_come_before_any_device_use():
    L = sa.lib()
    site = np.zeros(1, dtype=sa.TRAIN_SITE_DTYPE)
    assert L.sa_kmer_table_set_positions(None, site.ctypes.data, 1) == -1
    assert L.sa_kmer_table_add_batch_at(None, None, None, 0, 0, None, None) == -1
    sp, cp, n = C.c_void_p(), C.c_void_p(), np.zeros(1, dtype=np.int64)
    assert L.sa_kmer_table_position_counts(None, C.byref(sp), C.byref(cp), n.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    assert L.sa_kmer_table_add_at_times(None, None) == -1


ONE = ["-T", MODEL, "-q", NPREAD, "-p", "none.cigar", "-f", "none.fa", "-n", "chr"]
REFUSALS = [
    (["--train-positions", "none.positions"], "signalMachine: --train-positions needs a --train-* output"),
    (["--train-assignments", "{tmp}/a.tsv", "--train-positions-coverage", "{tmp}/c.tsv"],
     "signalMachine: --train-positions-coverage needs --train-positions <file>"),
    (["--train-assignments", "{tmp}/a.tsv", "--train-positions", "none.positions", "--rna"],
     "signalMachine: --train-positions does not take --rna runs"),
]


def test_the_three_refusals_and_the_usage_text(tmp_path):
    for more, message in REFUSALS:
        argv = [BIN] + ONE + [a.replace("{tmp}", str(tmp_path)) for a in more]
        pr = subprocess.run(argv, capture_output=True, text=True, timeout=60)
        err = pr.stderr.splitlines()
        assert pr.returncode == 1, (more, pr.stderr[-500:])
        assert err[-1] == message, err[-1]
        assert len(err) == 104                                            # the usage text, then the refusal
        assert not os.listdir(tmp_path)
    pr = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert len(pr.stderr.splitlines()) == 103
    assert "--train-positions <positions.tsv>" in pr.stderr and "--train-positions-coverage <file>" in pr.stderr
