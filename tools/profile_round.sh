#!/bin/bash
# Collects what profiles/ holds for a round: bench JSON (with cpu_baseline), rocprofv3 kernel stats of the same command,
# and the two PMC passes for HBM traffic.  usage (on the GPU box): [OUT=<dir>] bash tools/profile_round.sh <tag>  -> <dir>/<tag> (default prof_out/<tag>)
tag=$1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
o=${OUT:-prof_out}/$tag
mkdir -p $o
if [ -z "$SKIP_BENCH" ]; then ( time timeout 900 python bench.py --full ) > $o/bench.json 2> $o/bench.err; tail -c 600 $o/bench.json; fi
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $o/stats -o k -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-parity-mode --no-reference-loop --no-power --no-ek100 --no-small-batch --no-separate-update > $o/stats.log 2>&1
find $o/stats -name "*kernel_trace.csv" -delete
timeout 900 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $o/pmc_fetch -o f -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-parity-mode --no-reference-loop --no-power --no-ek100 --no-small-batch --no-separate-update > $o/pmc_fetch.log 2>&1
timeout 900 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $o/pmc_write -o w -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-parity-mode --no-reference-loop --no-power --no-ek100 --no-small-batch --no-separate-update > $o/pmc_write.log 2>&1
python tools/traffic_summary.py $o/pmc_fetch $o/pmc_write $o/traffic.json cfg2 64 bf16 1 > /dev/null
find $o -name "*counter_collection.csv" -delete
ls -R $o | head -30
