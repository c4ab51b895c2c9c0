"""signalMachine --batch on a few hundred reads, single-nucleotide probabilities two ways: one run with --snp-step N (posteriors
'-'), and the reference's route of N runs with -s 0 on FASTAs with X at the positions = s (mod N), each writing its TSVs.  The
bundled 1-D read, R9.4 6-mer model, aligned in windows at staggered offsets.  Prints one JSON line with the wall times."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sa_oracle_py as oracle  # noqa: E402

N_READS = int(sys.argv[1]) if len(sys.argv) > 1 else 300
STEP = int(sys.argv[2]) if len(sys.argv) > 2 else 10
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
GOLD = os.path.join(ROOT, "tests", "golden")
npread = os.path.join(GOLD, "npReads", "r9p4_oneD.npRead")
read = oracle.parse_npread(npread)["template_read"]
L = 1500
d = tempfile.mkdtemp()


def fasta(path, seq):
    with open(path, "w") as f:
        f.write(">chrA\n%s\n" % seq)
    with open(path + ".fai", "w") as f:
        f.write("chrA\t%d\t6\t%d\t%d\n" % (len(seq), len(seq), len(seq) + 1))


fasta(os.path.join(d, "ref.fa"), read)
for s in range(STEP):
    fasta(os.path.join(d, "ref_%d.fa" % s), "".join("X" if i % STEP == s else c for i, c in enumerate(read.upper())))
span = max(1, len(read) - L - 1)
man_dash, man_s = [], [[] for _ in range(STEP)]
for i in range(N_READS):
    o = (i * 37) % span
    cg = os.path.join(d, "g%d.cigar" % i)
    with open(cg, "w") as f:
        f.write("cigar: r%d %d %d + chrA %d %d + 1 M %d\n" % (i, o, o + L, o, o + L, L))
    man_dash.append("r%d\t%s\t%s\t-\n" % (i, npread, cg))
    for s in range(STEP):
        man_s[s].append("r%d\t%s\t%s\t%s\n" % (i, npread, cg, os.path.join(d, "s%d_r%d.tsv" % (s, i))))
open(os.path.join(d, "m_dash"), "w").writelines(man_dash)
for s in range(STEP):
    open(os.path.join(d, "m_%d" % s), "w").writelines(man_s[s])
base = [BIN, "-T", os.path.join(GOLD, "models", "testModelR9.4_450bps.nucleotide.6mer.template.model"), "-n", "chrA", "-g", "100"]


def run(args):
    t0 = time.perf_counter()
    pr = subprocess.run(base + args, capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        print(pr.stderr[-2000:], file=sys.stderr)
        sys.exit(1)
    return time.perf_counter() - t0


res = {"reads": N_READS, "step": STEP, "events_per_read": "about %d" % int(L * 1.67)}
t_snp = run(["-f", os.path.join(d, "ref.fa"), "--batch", os.path.join(d, "m_dash"), "--snp-step", str(STEP), "--snp-dir",
             os.path.join(d, "snp")])
t_runs = [run(["-f", os.path.join(d, "ref_%d.fa" % s), "--batch", os.path.join(d, "m_%d" % s), "-s", "0"]) for s in range(STEP)]
res["snp_step_wall_s"] = round(t_snp, 3)
res["s0_runs_wall_s"] = round(sum(t_runs), 3)
res["per_s0_run_wall_s"] = [round(t, 3) for t in t_runs]
res["speedup"] = round(sum(t_runs) / t_snp, 2)
res["files"] = len(os.listdir(os.path.join(d, "snp")))
print(json.dumps(res))
