"""Writes tests/golden/cigars/r9p4_oneD_bwa.json: the alignment `bwa mem -x ont2d` made of the template read of
tests/golden/npReads/r9p4_oneD.npRead, as the reference ships it (run in the build container, where /root/reference exists).  The
fixture is data: the first record's FLAG, POS and CIGAR of tests/minion_test_reads/oneD_alignments.sam.  Its SEQ is the template
read of the bundled .npRead (asserted here), and POS - 1 is the first position of the window that
tests/golden/expected/reference_output_ecoli1d.npz holds.  It is the alignment that file was written with (together with
traceBackDiagonals = 40 and an A at the window's one unknown base): tests/sa_cases.py parses it -- leading S = read start 42, M/D/I =
operations 0/1/2 -- and with it all of the file's rows are reproduced."""
import json
import os

import numpy as np

SAM = "/root/reference/tests/minion_test_reads/oneD_alignments.sam"
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    rec = next(l for l in open(SAM) if not l.startswith("@")).rstrip("\n").split("\t")
    read = open(os.path.join(HERE, "npReads", "r9p4_oneD.npRead")).read().split("\n")[2].split()[0]
    assert rec[9] == read, "the SAM record's SEQ is not the template read of r9p4_oneD.npRead"
    z = np.load(os.path.join(HERE, "expected", "reference_output_ecoli1d.npz"))
    assert int(rec[3]) - 1 == int(z["first_position"])
    out = dict(source="tests/minion_test_reads/oneD_alignments.sam, first record (bwa mem -x ont2d)", query=rec[0], flag=int(rec[1]),
               contig=rec[2], pos=int(rec[3]), cigar=rec[5])
    with open(os.path.join(HERE, "cigars", "r9p4_oneD_bwa.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
