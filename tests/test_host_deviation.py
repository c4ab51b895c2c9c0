"""CPU checks of the guide-deviation stage (sa_batch_guide_deviation, sa_guide_deviation_records): header, export list and ctypes
agree on the new names, every refused argument is refused before the device is looked for, and the restatement in deviation_ref.py
gives a hand-worked answer."""
import ctypes as C
import re

import signalalign_amd as sa
from signalalign_amd import _capi

from abi_header import header_text

import deviation_ref as ref

NEW = ["sa_batch_guide_deviation", "sa_guide_deviation_records", "sa_guide_deviation_release"]


def test_header_exports_and_ctypes_agree():
    hdr = header_text()
    declared = set(re.findall(r"\b(sa_(?:batch_)?guide_deviation[a-z0-9_]*)\s*\(", hdr))
    assert set(NEW) == declared
    assert declared <= set(_capi.EXPORTS)
    L = sa.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        n_params = 0 if decl.strip() == "void" else len(decl.split(","))
        assert len(fn.argtypes) == n_params, name
    assert _capi.DEVIATION_READ_DTYPE.itemsize == 64 and _capi.DEVIATION_SET_DTYPE.itemsize == 32
    assert _capi.DEVIATION_EVENT_DTYPE.itemsize == 16 and C.sizeof(_capi.DeviationJob) == 32 and C.sizeof(_capi.DeviationParams) == 12
    for name in ("DEV_NO_GUIDE", "DEV_NO_RECORDS", "DEV_DIRECT", "DEV_EVENTS", "DEV_WINDOW"):
        assert getattr(sa, name) == int(re.search(r"#define SA_%s (\d+)u?\b" % name, hdr).group(1)), name


JOB = dict(ax=[10, 15, 30], ay=[2, 5, 8], n_events=11)
GOOD = dict(jobs=[JOB], first=[0, 2], x=[3, 4], y=[0, 10], prob_e7=[0, 10 ** 7], mea=[[(0, 0), (1, 10)]], params=(10, 5, 64))


def _code(**change):
    a = dict(GOOD, **change)
    try:
        sa.guide_deviation_records(a["jobs"], a["first"], a["x"], a["y"], a["prob_e7"], mea=a["mea"], params=a["params"])
    except sa.SaError as e:
        return e.code
    return 0


def test_refusals_come_before_the_device():
    accepted = 0 if sa.device_count() > 0 else -3                        # SA_ENODEVICE: nothing wrong with the arguments
    assert _code() == accepted
    assert _code(mea=None) == accepted
    assert _code(params=None) == accepted
    bad = [
        dict(jobs=[dict(JOB, ay=[2, 2, 8])]),                            # anchor_y not strictly increasing
        dict(jobs=[dict(JOB, ay=[5, 2, 8])]),
        dict(jobs=[dict(JOB, ax=[-1, 15, 30])]),                         # anchor_x outside [0, 2^28)
        dict(jobs=[dict(JOB, ax=[10, 15, 2 ** 28])]),
        dict(y=[0, 11]), dict(y=[-1, 10]),                               # a record outside [0, n_events)
        dict(x=[-1, 4]), dict(x=[3, 2 ** 28]),
        dict(mea=[[(0, 11)]]), dict(mea=[[(0, -1)]]),                    # an MEA event outside [0, n_events)
        dict(prob_e7=[-1, 5]), dict(prob_e7=[5, 10 ** 7 + 1]),
        dict(params=(-1, 5, 64)),                                        # threshold < 0
        dict(params=(10, 0, 64)),                                        # bucket_size < 1
        dict(params=(10, 5, 0)), dict(params=(10, 5, 1025)),             # n_buckets outside [1, 1024]
        dict(jobs=[dict(JOB, n_events=-1)], y=[0, 0], mea=None),
    ]
    for change in bad:
        assert _code(**change) == -1, change
    # the edges that are allowed
    ok = [dict(params=(0, 1, 1)), dict(params=(10, 5, 1024)), dict(jobs=[dict(JOB, ax=[0, 15, 2 ** 28 - 1])]),
          dict(jobs=[dict(ax=[], ay=[], n_events=11)])]
    for change in ok:
        assert _code(**change) == accepted, change
    for flags in (8, sa.DEV_DIRECT | sa.DEV_WINDOW):                     # an unknown flag; the two paths at once
        try:
            sa.guide_deviation_records([JOB], [0, 0], [], [], [], flags=flags)
            assert False, flags
        except sa.SaError as e:
            assert e.code == -1
    L = sa.lib()
    assert L.sa_batch_guide_deviation(None, None, 0, None, None, None, 0, None, None, None, None, None, None, None) == -1


# The hand-worked read: anchors (10, 2), (15, 5), (30, 8), eleven events, threshold 10, buckets of 5, five of them.
#   y  guide                        records (x, prob_e7)        best  diff  abs
#   0  10  before the first anchor  (10, 5)                      10     0    0
#   1  10  before the first anchor  (9, 5)                        9    -1    1
#   2  10  on an anchor             (12, 500) (30, 900)          30    20   20  flagged
#   3  12  (10 + 15) / 2, odd sum   (40, 1)                      40    28   28  flagged, on the path
#   4  12  ...                      none: unaligned, inside the run and on the path
#   5  15  on an anchor             (30, 7)                      30    15   15  flagged
#   6  22  (15 + 30) / 2, odd sum   (22, 7)                      22     0    0  closes the run 2..5
#   7  22                           (20, 700) (25, 700) a tie    25     3    3
#   8  30  on an anchor             (30, 7) (30, 9) same (x, y)  30     0    0
#   9  30  after the last anchor    (5, 7)                        5   -25   25  flagged
#  10  30  after the last anchor    (50, 7)                      50    20   20  flagged, on the path: the run is open at the end
HAND = [(10, 0, 5), (9, 1, 5), (12, 2, 500), (30, 2, 900), (40, 3, 1), (30, 5, 7), (22, 6, 7), (20, 7, 700), (25, 7, 700), (30, 8, 7),
        (30, 8, 9), (5, 9, 7), (50, 10, 7)]


def test_known_answer_of_the_restatement():
    x, y, p = [list(c) for c in zip(*HAND)]
    got = ref.deviation([JOB], [0, len(x)], x, y, p, mea=[[3, 4, 10]], threshold=10, bucket_size=5, n_buckets=5)
    rows = got["rows"][0]
    assert [r["y"] for r in rows] == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10]
    assert [r["guide"] for r in rows] == [10, 10, 10, 12, 15, 22, 22, 30, 30, 30]
    assert [r["best_x"] for r in rows] == [10, 9, 30, 40, 30, 22, 25, 30, 5, 50]
    assert [r["diff"] for r in rows] == [0, -1, 20, 28, 15, 0, 3, 0, -25, 20]
    assert [r["flagged"] for r in rows] == [False, False, True, True, True, False, False, False, True, True]
    assert [r["y"] for r in rows if r["on_mea"]] == [3, 10]
    assert got["hist"] == [[5, 0, 0, 1, 4]] and got["total_hist"] == [5, 0, 0, 1, 4]
    assert got["sets"] == [
        dict(first_event=2, last_event=5, count=3, peak=28, mea_peak=28, center_event=3, open_end=0),
        dict(first_event=9, last_event=10, count=2, peak=25, mea_peak=20, center_event=9, open_end=1)]
    assert got["reads"] == [dict(status=0, n_sets=2, set_first=0, n_aligned=10, n_flagged=5, n_on_mea=2, sum_abs=112, max_abs=28,
                                 max_abs_mea=28, max_event=3)]
    # the reference's list: the set that is open at the end is never emitted there
    like_ref = ref.deviation([JOB], [0, len(x)], x, y, p, mea=[[3, 4, 10]], n_buckets=5, drop_open_sets=True)
    assert like_ref["sets"] == [s for s in got["sets"] if not s["open_end"]] and like_ref["reads"][0]["n_sets"] == 1
    # row order does not matter, nor do the statuses of jobs without a guide or without records disturb their neighbours
    rev = ref.deviation([dict(ax=[], ay=[], n_events=11), JOB, JOB], [0, len(x), 2 * len(x), 2 * len(x)], (x + x)[::-1], (y + y)[::-1],
                        (p + p)[::-1], n_buckets=5)
    assert [r["status"] for r in rev["reads"]] == [ref.NO_GUIDE, 0, ref.NO_RECORDS]
    assert rev["reads"][0]["n_aligned"] == 0 and rev["rows"][0] == [] and rev["hist"][0] == [0] * 5
    assert rev["reads"][1]["set_first"] == 0 and rev["sets"] == [dict(s, mea_peak=0) for s in got["sets"]]
