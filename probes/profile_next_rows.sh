#!/bin/bash
# rocprofv3 kernel statistics of the two "next" rows and of the headline bench, same commands
# as bench.py --full runs them.  Output under $OUT (default bench_out/); the summaries worth keeping are copied to profiles/ by hand.
set -e
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_ea -- python3 bench.py --full --workload event_align --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_ea.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_mea -- python3 bench.py --full --workload mea --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_mea.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_main -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_main.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_real -- python3 bench.py --full --workload realistic --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_real.log 2>&1
python3 bench.py --full > $OUT/bench_main.json 2> $OUT/bench_main.err
python3 bench.py --full --workload event_align > $OUT/bench_ea.json 2> $OUT/bench_ea.err
python3 bench.py --full --workload mea > $OUT/bench_mea.json 2> $OUT/bench_mea.err
python3 bench.py --full --workload realistic > $OUT/bench_real.json 2> $OUT/bench_real.err
echo done
