"""Writes tests/golden/raw/*.npz: raw current of three reads of the reference's test tree, for the event detector's
known-answer tests (tests/test_host_event_detect.py, tests/test_gpu_event_detect.py).  Runs only in the build container,
where /root/reference exists, with libhdf5 at /opt/conda/lib (read through ctypes; no Python HDF5 package needed).  The
fixtures are data: the int16 samples of Raw/Reads/Read_*/Signal, the f64 bit patterns of the five attributes the
reference reads (through H5T_NATIVE_FLOAT, so the product takes them as floats) and the read id.

  read61_rna    RNA_no_events/...read_61_ch_151...      (the reference's tests name it under RNA_edge_cases/)
  read108_dna   1D/...ch112_read108...                   (the read behind tests/golden/npReads/r9p4_oneD.npRead)
  read1108_dna  embedded_files/...ch92_read1108...       (extra real signal, bit parity only)

Also copies models/testModelR9p4_5mer_acgt_RNA.model to tests/golden/models/ and writes the @8898d755 record of
RNA_edge_cases/rna_reads.fastq (the sequence the reference's RNA tests spell out) to tests/golden/raw/rna_8898d755.txt.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

REF = "/root/reference"
READS = os.path.join(REF, "tests", "minion_test_reads")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "raw")
H5DUMP = "/opt/conda/bin/h5dump"
LIBHDF5 = "/opt/conda/lib/libhdf5.so"

FILES = {
    "read61_rna": ("RNA_no_events", "read_61_ch_151"),
    "read108_dna": ("1D", "ch112_read108"),
    "read1108_dna": ("embedded_files", "ch92_read1108"),
}


class H5:
    def __init__(self):
        L = C.CDLL(LIBHDF5)
        L.H5open()
        hid = C.c_int64
        for f in ("H5Fopen", "H5Dopen2", "H5Aopen_by_name"):
            getattr(L, f).restype = hid
        L.H5Fopen.argtypes = [C.c_char_p, C.c_uint, hid]
        L.H5Dopen2.argtypes = [hid, C.c_char_p, hid]
        L.H5Aopen_by_name.argtypes = [hid, C.c_char_p, C.c_char_p, hid, hid]
        L.H5Dread.argtypes = [hid, hid, hid, hid, hid, C.c_void_p]
        L.H5Aread.argtypes = [hid, hid, C.c_void_p]
        L.H5Dclose.argtypes = L.H5Aclose.argtypes = L.H5Fclose.argtypes = [hid]
        self.L = L
        self.short = hid.in_dll(L, "H5T_NATIVE_SHORT_g").value
        self.double = hid.in_dll(L, "H5T_NATIVE_DOUBLE_g").value

    def signal(self, f, path, n):
        d = self.L.H5Dopen2(f, path.encode(), 0)
        assert d >= 0, path
        buf = np.zeros(n, dtype=np.int16)
        assert self.L.H5Dread(d, self.short, 0, 0, 0, buf.ctypes.data) >= 0
        self.L.H5Dclose(d)
        return buf

    def attr_f64(self, f, obj, name):
        a = self.L.H5Aopen_by_name(f, obj.encode(), name.encode(), 0, 0)
        assert a >= 0, (obj, name)
        v = C.c_double()
        assert self.L.H5Aread(a, self.double, C.byref(v)) >= 0
        self.L.H5Aclose(a)
        return v.value


def find(sub, key):
    d = os.path.join(READS, sub)
    hits = [f for f in os.listdir(d) if key in f and f.endswith(".fast5")]
    assert len(hits) == 1, (sub, key, hits)
    return os.path.join(d, hits[0])


def main():
    os.makedirs(OUT, exist_ok=True)
    h = H5()
    for name, (sub, key) in FILES.items():
        path = find(sub, key)
        listing = subprocess.check_output([H5DUMP, "-n", path]).decode()
        group = re.search(r"dataset\s+(/Raw/Reads/Read_\d+)/Signal", listing).group(1)
        header = subprocess.check_output([H5DUMP, "-H", "-d", group + "/Signal", path]).decode()
        n = int(re.search(r"DATASPACE\s+SIMPLE\s+\{\s*\(\s*(\d+)", header).group(1))
        rid = subprocess.check_output([H5DUMP, "-a", group + "/read_id", path]).decode()
        read_id = re.search(r'\(0\): "([^"]+)"', rid).group(1)
        f = h.L.H5Fopen(path.encode(), 0, 0)
        assert f >= 0, path
        raw = h.signal(f, group + "/Signal", n)
        ch = "/UniqueGlobalKey/channel_id"
        attrs = np.array([h.attr_f64(f, ch, "digitisation"), h.attr_f64(f, ch, "offset"), h.attr_f64(f, ch, "range"),
                          h.attr_f64(f, ch, "sampling_rate"), h.attr_f64(f, group, "start_time")], dtype=np.float64)
        h.L.H5Fclose(f)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), raw=raw, attrs_f64_bits=attrs.view(np.uint64),
                            attr_names=np.array(["digitisation", "offset", "range", "sampling_rate", "start_time"]),
                            read_id=np.array(read_id), source=np.array(os.path.relpath(path, READS)))
        print(name, n, read_id, attrs)
    shutil.copy(os.path.join(REF, "models", "testModelR9p4_5mer_acgt_RNA.model"), os.path.join(HERE, "models"))
    lines = open(os.path.join(READS, "RNA_edge_cases", "rna_reads.fastq")).read().split("\n")
    i = next(i for i, l in enumerate(lines) if l.startswith("@8898d755"))
    with open(os.path.join(OUT, "rna_8898d755.txt"), "w") as fo:
        fo.write(lines[i + 1].strip() + "\n")


if __name__ == "__main__":
    if os.path.isdir(REF):
        main()
