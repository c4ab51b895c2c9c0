"""Reads from raw current, the host side (no GPU): the raw-read file (signalalign_amd/rawio.py and the C loader
sa_rawread_load), the restatement of NanoporeRead.make_event_map (tests/raw_npread_ref.py) on hand-built tables, the argument
checks of sa_npread_from_raw_batch that need no device, and the header / EXPORTS / ctypes agreement for the new symbols."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi, rawio

from abi_header import header_text

import raw_npread_ref as N
import sa_cases as cases
from test_host_event_detect import DNA_MODEL, dna_sequence, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sa_npread_from_raw_batch", "sa_raw_npread_free", "sa_raw_npread_write", "sa_npread_last_finish_ms")


def test_header_exports_and_mirror_agree_on_the_new_symbols():
    hdr = header_text()
    L = sa.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr) and name in _capi.EXPORTS and hasattr(L, name), name
    for name in ("sa_rawread_load", "sa_rawread_free", "sa_rawread_is"):     # the CLI's loader: csrc/sa_io.h
        assert hasattr(L, name), name
    assert re.search(r"#define SA_RAW_MAP_LENGTH 32\b", hdr) and sa.RAW_MAP_LENGTH == 32
    # the struct the header declares, field for field
    body = re.search(r"typedef struct sa_raw_npread \{(.*?)\} sa_raw_npread_t;", hdr, flags=re.S).group(1)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1])]
    assert declared == [f[0] for f in _capi.RawNpRead._fields_], declared


def _read108():
    f = fixture("read108_dna")
    a = np.asarray(f["attrs_f64_bits"], dtype=np.uint64).view(np.float64)
    return dict(raw=f["raw"], digitisation=a[0], offset=a[1], range=a[2], sample_rate=a[3], start_time=a[4])


def test_rawio_round_trip_and_the_c_loader(tmp_path):
    job, seq = _read108(), dna_sequence()
    p = str(tmp_path / "read108.saraw")
    rawio.write_raw(p, sequence=seq, **job)
    assert rawio.is_raw(p) and not rawio.is_raw(DNA_MODEL) and sa.lib().sa_rawread_is(p.encode()) == 1
    assert os.path.getsize(p) == 8 + 20 + 16 + len(seq) + 2 * len(job["raw"])
    for got in (rawio.read_raw(p), sa.rawread_load(p)):
        assert np.array_equal(got["raw"], job["raw"]) and got["raw"].dtype == np.int16 and got["sequence"] == seq
        for f in ("digitisation", "offset", "range", "sample_rate", "start_time"):
            assert np.float32(got[f]) == np.float32(job[f]), f
    # an empty sequence and one sample are a legal file (the caller refuses a sequence shorter than k)
    q = str(tmp_path / "tiny.saraw")
    rawio.write_raw(q, np.array([7], dtype=np.int16), 8192.0, 1.0, 1400.0, 4000.0, 0.0, "")
    got = sa.rawread_load(q)
    assert got["raw"].tolist() == [7] and got["sequence"] == "" and got["range"] == 1400.0


def test_loader_rejects(tmp_path):
    job, seq = _read108(), dna_sequence()[:300]
    job["raw"] = job["raw"][:3000]
    good = str(tmp_path / "good.saraw")
    rawio.write_raw(good, sequence=seq, **job)
    data = open(good, "rb").read()
    head = 8 + 20 + 16

    def refused(name, blob, code):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(blob)
        with pytest.raises(sa.SaError) as ei:
            sa.rawread_load(p)
        assert ei.value.code == code, (name, ei.value.code)
        with pytest.raises(ValueError):
            rawio.read_raw(p)

    refused("magic.saraw", b"SARAW2\0\0" + data[8:], -1)                          # SA_EINVAL
    refused("cut_samples.saraw", data[:head + len(seq) + 2 * 1000 + 1], -6)     # SA_EIO: cut inside the samples
    refused("cut_header.saraw", data[:30], -6)
    refused("cut_sequence.saraw", data[:head + 10], -6)
    refused("longer.saraw", data + b"\0\0", -6)
    refused("no_samples.saraw", data[:28] + struct.pack("<qq", 0, len(seq)) + data[head:head + len(seq)], -1)
    refused("too_many.saraw", data[:28] + struct.pack("<qq", 2 ** 31, len(seq)) + data[head:], -1)
    refused("negative_seq.saraw", data[:28] + struct.pack("<qq", 3000, -1) + data[head:], -1)
    with pytest.raises(sa.SaError) as ei:
        sa.rawread_load(str(tmp_path / "missing.saraw"))
    assert ei.value.code == -6
    with pytest.raises(ValueError):
        rawio.write_raw(str(tmp_path / "empty.saraw"), np.zeros(0, dtype=np.int16), 1.0, 0.0, 1.0, 4000.0, 0.0, "ACGT")


@pytest.mark.parametrize("move, prob, expect", [
    ([0, 1, 1, 1], [.5, .5, .5, .5], [0, 1, 2, 3]),                      # all moves 1 (row 0's move does not count)
    ([0, 1, 3, 1], [.5, .5, .5, .5], [0, 1, 1, 1, 2, 3]),                # a move of 3: two copies of the row before
    ([0, 1, 1, 0, 1], [.5, .5, .2, .9, .5], [0, 1, 3, 4]),               # move 0, higher probability: replaces
    ([0, 1, 1, 0, 1], [.5, .5, .9, .9, .5], [0, 1, 2, 4]),               # equal: does not
    ([0, 1, 1, 0, 1], [.5, .5, .9, .2, .5], [0, 1, 2, 4]),               # lower: does not
    ([0, 0, 1], [.5, .1, .5], [1, 2]),                                   # row 1 is compared with 0, not with row 0
    ([2, 1], [.5, .5], [0, 1]),                                          # row 0's own move is ignored
    ([0], [.5], [0]),                                                    # a single row
])
def test_make_event_map_on_hand_built_tables(move, prob, expect):
    for k in (1, 5, 6):
        got = N.make_event_map(np.array(move), np.array(prob), k)
        assert got == expect + [expect[-1]] * (k - 1), (k, got)
        assert len(got) == 1 + sum(move[1:]) + (k - 1)


def test_writer_layout_on_a_hand_built_table():
    rows = np.zeros(3, dtype=sa.RAW_EVENT_DTYPE)
    rows["mean"], rows["stdv"], rows["length"] = [80.5, 90.25, 100.0], [1.0, 1.5, 0.1], [0.001, 0.002, 0.00125]
    rows["start"], rows["kmer_idx"], rows["move"], rows["p_model_state"] = [10.0, 10.001, 10.003], [0, 1, 3], [0, 1, 2], [.5, 1e-5, .25]
    text = N.npread_text("ACGTACGT", rows, 5)
    lines = text.split("\n")
    assert len(lines) == 15 and lines[14] == ""
    assert lines[0] == "0 3 0 8 0 1 1 1 1 1 0 1 1 1 1 1 0 0" and lines[1] == "" and lines[2] == "ACGTACGT"
    assert lines[3] == "0 1 1 2 2 2 2 2 "
    assert lines[7].startswith("80.5 1.0 0.001 0.0 90.25 1.5 0.002 ") and lines[7].endswith(" ")
    assert lines[10] == "ACGTA CGTAC TACGT " and lines[11] == "0.5 1e-05 0.25 "
    assert [lines[i] for i in (4, 5, 6, 8, 9, 12, 13)] == [""] * 7
    # the bundled 1D .npRead has the same first line but for its event count, and the same empty lines
    ref = open(os.path.join(ROOT, "tests", "golden", "npReads", "r9p4_oneD.npRead")).read().split("\n")
    assert ref[0] == "0 10922 0 6542 0 1 1 1 1 1 0 1 1 1 1 1 0 0" and len(ref) == 15
    assert [ref[i] for i in (1, 4, 5, 6, 8, 9, 12, 13, 14)] == [""] * 9 and ref[3].endswith(" ") and ref[10].endswith(" ")


def test_argument_checks_need_no_device():
    L = sa.lib()
    m = sa.Model.load(DNA_MODEL)
    raw = np.arange(100, dtype=np.int16)
    job = _capi.RawJob(raw.ctypes.data_as(C.POINTER(C.c_int16)), 100, 8192.0, 0.0, 1400.0, 4000.0, 0.0)
    jobs = (_capi.RawJob * 1)(job)
    seqs = (C.c_char_p * 1)(b"ACGTACGTACGT")
    out = (_capi.RawNpRead * 1)()
    call = L.sa_npread_from_raw_batch
    assert call(None, jobs, seqs, 1, None, 0, 0, out, None) == -1
    assert call(m._h, None, seqs, 1, None, 0, 0, out, None) == -1
    assert call(m._h, jobs, None, 1, None, 0, 0, out, None) == -1
    assert call(m._h, jobs, seqs, 1, None, 0, 0, None, None) == -1
    assert call(m._h, jobs, seqs, -1, None, 0, 0, out, None) == -1
    assert call(m._h, jobs, seqs, 1, None, 0, sa.FLAG_RNA, out, None) == -8          # SA_EUNSUPPORTED
    hdp = sa.Model.load(cases.MODEL_R73, cases.NHDP)
    assert call(hdp._h, jobs, seqs, 1, None, 0, 0, out, None) == -8
    # per-read checks: no samples, a sequence shorter than k, a NULL sequence, a detector window of 0
    empty = (_capi.RawJob * 1)(_capi.RawJob(raw.ctypes.data_as(C.POINTER(C.c_int16)), 0, 8192.0, 0.0, 1400.0, 4000.0, 0.0))
    assert call(m._h, empty, seqs, 1, None, 0, 0, out, None) == -1
    assert call(m._h, jobs, (C.c_char_p * 1)(b"ACGT"), 1, None, 0, 0, out, None) == -1
    assert call(m._h, jobs, (C.c_char_p * 1)(None), 1, None, 0, 0, out, None) == -1
    assert call(m._h, jobs, seqs, 1, C.byref(_capi.DetectorParams(0, 6, 1.4, 9.0, 0.2)), 0, 0, out, None) == -1
    assert out[0].status == 0 and not out[0].events4
    if sa.device_count() == 0:
        assert call(m._h, jobs, seqs, 1, None, 0, 0, out, None) == -3                # then SA_ENODEVICE, never a fallback
    # the writer refuses a read that failed
    out[0].status = 1
    assert L.sa_raw_npread_write(C.byref(out[0]), b"ACGTACGTACGT", m._h, b"/dev/null") == -1
    L.sa_raw_npread_free(out, 1)
    assert L.sa_npread_last_finish_ms() >= 0.0
