"""Call scores, the host side (no GPU): the header, EXPORTS and the ctypes mirror agree; the restatement (call_scores_ref.py) gives
hand-computed answers; sa_call_scores_write prints the restatement's text byte for byte; the device entry points refuse loudly."""
import ctypes as C
import re

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi

from abi_header import header_text

import call_scores_ref as ref

NEW = ["sa_sort_u64", "sa_call_scores_create", "sa_call_scores_destroy", "sa_call_scores_add_batch", "sa_call_scores_add_records",
       "sa_call_scores_checkpoint", "sa_call_scores_rollback", "sa_call_scores_finish", "sa_call_scores_write"]


def test_header_exports_and_ctypes_agree():
    hdr = header_text()
    declared = set(re.findall(r"\b(sa_(?:sort|call_scores)_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) == declared
    assert declared <= set(_capi.EXPORTS)
    L = sa.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(fn.argtypes) == len(decl.split(",")), name
    assert sa.SORT_TILE == int(re.search(r"#define SA_SORT_TILE (\d+)\b", hdr).group(1))
    # structure layouts: the header's fields in order, the mirrors' sizes
    for struct, names, size in (("sa_truth_site", sa.TRUTH_SITE_DTYPE.names, 24), ("sa_call_score_row", sa.CALL_SCORE_ROW_DTYPE.names, 80),
                                ("sa_score_job_map", [f for f, _ in sa.ScoreJobMap._fields_], 32),
                                ("sa_call_scores_counts", [f for f, _ in _capi.CallScoresCounts._fields_], 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), hdr, flags=re.S).group(1)
        fields = [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip()
                  for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == list(names), struct
    assert sa.TRUTH_SITE_DTYPE.itemsize == C.sizeof(sa.TruthSite) == 24 and sa.CALL_SCORE_ROW_DTYPE.itemsize == 80
    assert C.sizeof(sa.ScoreJobMap) == 32 and C.sizeof(_capi.CallScoresCounts) == 16
    assert sa.CALL_SCORE_ROW_DTYPE.fields["auc2"][1] == 32 and sa.CALL_SCORE_ROW_DTYPE.fields["tp"][1] == 48
    assert hasattr(sa.CallScores, "add_batch") and hasattr(sa.CallScores, "add_records") and hasattr(sa.CallScores, "finish")


POS = [0.9, 0.5, 0.5, 0.2]
NEG = [0.5, 0.2, 0.2, 0.1]


def test_restatement_on_eight_scores_with_ties():
    """By hand: p = 0.9 has 4 negatives below it (8); each p = 0.5 has 3 below and 1 equal (7 each); p = 0.2 has 1 below and 2 equal (4):
    auc2 = 8 + 14 + 4 = 26 of 2 * 4 * 4 = 32.  The same as the trapezoid area under the ROC points (0, 0), (0, 1/4), (1/4, 3/4),
    (3/4, 1), (1, 1) over the distinct thresholds 0.9, 0.5, 0.2, 0.1: 1/4 * (1/4 + 3/4) / 2 + 1/2 * (3/4 + 1) / 2 + 1/4 = 13/16."""
    r = ref.row(POS, NEG, 4, 0.5)
    assert r["auc2"] == 26 and r["auc"] == 26.0 / 32.0 == 13.0 / 16.0
    assert (r["n_pos"], r["n_neg"], r["tp"], r["fp"], r["fn"], r["tn"]) == (4, 4, 3, 1, 1, 3)
    assert r["tp_ge"] == [4, 3, 3, 1, 0] and r["fp_ge"] == [4, 1, 1, 0, 0]
    r = ref.row(POS, NEG, 4, 0.500000001)
    assert (r["tp"], r["fp"], r["fn"], r["tn"]) == (1, 0, 3, 4)
    # the explicit trapezoid over the distinct thresholds, in exact fractions
    from fractions import Fraction
    pts = [(Fraction(0), Fraction(0))]
    for t in sorted(set(POS + NEG), reverse=True):
        pts.append((Fraction(sum(v >= t for v in NEG), 4), Fraction(sum(v >= t for v in POS), 4)))
    area = sum((x1 - x0) * (y0 + y1) / 2 for (x0, y0), (x1, y1) in zip(pts, pts[1:]))
    assert area == Fraction(26, 32)
    # -0.0 is +0.0, a class without scores gives nan, the union of two strands has the cross terms
    assert ref.keys([-0.0, 0.0, 5e-324, 1.0]).tolist() == [0, 0, 1, 0x3FF0000000000000]
    assert np.isnan(ref.row([0.5], [], 4, 0.5)["auc"])
    assert ref.auc2([0.9], [0.1]) + ref.auc2([0.3], [0.6]) == 2 and ref.auc2([0.9, 0.3], [0.1, 0.6]) == 6
    assert ref.read_mean([0.1, 0.2, 0.3]) == ((0 + 0.1) + 0.2 + 0.3) / 3


def _rows_array(rows):
    out = np.zeros(len(rows), dtype=sa.CALL_SCORE_ROW_DTYPE)
    for o, r in zip(out, rows):
        for f in ("level", "group", "n_pos", "n_neg", "auc2", "auc", "tp", "fp", "tn", "fn"):
            o[f] = r[f]
        o["letter"] = r["letter"].encode()
    curves = np.array([[r["tp_ge"], r["fp_ge"]] for r in rows], dtype=np.int64)
    return out, curves


def test_write_matches_the_restatement_byte_for_byte(tmp_path):
    rng = np.random.default_rng(5)
    s = ref.Scores("CE", 7, 0.500000001)
    for level, strand, n in ((0, 0, 40), (0, 1, 25), (1, 0, 6), (2, 1, 9)):
        p = np.round(rng.random(n), 6 if level == 2 else 17)
        s.add_records(level, strand, np.stack([p, 1.0 - p], axis=1), rng.integers(0, 2, n))
    s.add(2, 0, [1.0, 0.0], 0)                                  # a class without negatives for C, without positives for E
    s.arr = {k: v for k, v in s.arr.items() if k[:2] != (1, 0) or k[3] == 1}   # level 1, t: positives only (auc nan)
    rows = s.rows()
    assert any(np.isnan(r["auc"]) for r in rows) and any(r["tp"] + r["fp"] == 0 for r in rows)
    arr, curves = _rows_array(rows)
    sp, cp = str(tmp_path / "summary.tsv"), str(tmp_path / "curves.tsv")
    sa.call_scores_write(sp, cp, 7, arr, curves)
    assert open(sp).read() == ref.summary_text(rows)
    assert open(cp).read() == ref.curves_text(rows, 7)
    sa.call_scores_write(sp, None, 7, arr)                      # the summary alone
    assert open(sp).read() == ref.summary_text(rows)
    with pytest.raises(sa.SaError) as e:
        sa.call_scores_write(str(tmp_path / "no" / "dir.tsv"), None, 7, arr)
    assert e.value.code == -6                                   # SA_EIO


def test_no_device_fails_loudly():
    if sa.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(sa.SaError) as e:
        sa.CallScores("CE", truth=[(0, 10, 0, "C")])
    assert e.value.code == -3                                   # SA_ENODEVICE
    with pytest.raises(sa.SaError) as e:
        sa.sort_u64(np.arange(10, dtype=np.uint64))
    assert e.value.code == -3
