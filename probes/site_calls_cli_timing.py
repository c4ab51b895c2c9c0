"""signalMachine --batch on a few hundred CpG reads, three ways: -s 0 alone; -s 0 with --site-calls-aggregate; and
--site-calls-aggregate with '-' posteriors (no TSV).  The bundled 1-D read, X at every CpG cytosine (-a X -> C/E), aligned in
windows at staggered offsets.  Prints one JSON line with the wall time and reads/s of each."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sa_oracle_py as oracle  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
GOLD = os.path.join(ROOT, "tests", "golden")
npread = os.path.join(GOLD, "npReads", "r9p4_oneD.npRead")
read = oracle.parse_npread(npread)["template_read"]
L = 1500
d = tempfile.mkdtemp()
ref = "".join("X" if read[i:i + 2] == "CG" else read[i] for i in range(len(read)))
with open(os.path.join(d, "ref.fa"), "w") as f:
    f.write(">chrA\n%s\n" % ref)
with open(os.path.join(d, "ref.fa.fai"), "w") as f:
    f.write("chrA\t%d\t6\t%d\t%d\n" % (len(ref), len(ref), len(ref) + 1))
with open(os.path.join(d, "ce"), "w") as f:
    f.write("X\tCE\n")
span = max(1, len(read) - L - 1)
man, man_dash = [], []
for i in range(N):
    s = (i * 37) % span
    cg = os.path.join(d, "g%d.cigar" % i)
    with open(cg, "w") as f:
        f.write("cigar: r%d %d %d + chrA %d %d + 1 M %d\n" % (i, s, s + L, s, s + L, L))
    man.append("r%d\t%s\t%s\t%s\n" % (i, npread, cg, os.path.join(d, "r%d.tsv" % i)))
    man_dash.append("r%d\t%s\t%s\t-\n" % (i, npread, cg))
open(os.path.join(d, "m"), "w").writelines(man)
open(os.path.join(d, "m_dash"), "w").writelines(man_dash)
base = [BIN, "-T", os.path.join(GOLD, "models", "testModelR9.4_450bps.cpg.6mer.template.model"), "-f", os.path.join(d, "ref.fa"),
        "-n", "chrA", "-s", "0", "-g", "100", "-a", os.path.join(d, "ce")]
res = {"reads": N, "events_per_read": "about %d" % int(L * 1.67)}
for name, extra in (("s0", ["--batch", os.path.join(d, "m")]),
                    ("s0_aggregate", ["--batch", os.path.join(d, "m"), "--site-calls-aggregate", os.path.join(d, "agg1")]),
                    ("aggregate_no_tsv", ["--batch", os.path.join(d, "m_dash"), "--site-calls-aggregate", os.path.join(d, "agg2")])):
    for f_ in os.listdir(d):
        if f_.endswith(".tsv"):
            os.remove(os.path.join(d, f_))
    t0 = time.perf_counter()
    pr = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
    dt = time.perf_counter() - t0
    if pr.returncode != 0:
        print(pr.stderr[-2000:], file=sys.stderr)
        sys.exit(1)
    res[name] = {"wall_s": round(dt, 3), "reads_per_s": round(N / dt, 1)}
res["aggregates_identical"] = open(os.path.join(d, "agg1")).read() == open(os.path.join(d, "agg2")).read()
print(json.dumps(res))
