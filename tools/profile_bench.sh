cd /tmp && export TMPDIR=/tmp
R=/root/repo
T=${ROUND:-r02}          # round tag: raw output under $OUT (default profile_out/$T), tools/refresh_profiles.py copies the summaries into profiles/
OUT=${OUT:-$R/profile_out/$T}
mkdir -p $OUT
python $R/bench.py --full > $OUT/bench.json 2> $OUT/bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python $R/bench.py --steps 200 --warmup 10 --no-cpu-baseline --no-secondary > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/fetch -- python $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/write -- python $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > /dev/null 2>&1
# C4-shaped workload (fused histogram): bench line + kernel stats
python $R/bench.py --workload rdf --steps 1024 --warmup 64 --full > $OUT/rdf_bench.json 2> $OUT/rdf_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/rdf_stats -- python $R/bench.py --workload rdf --steps 256 --warmup 32 --no-cpu-baseline > /dev/null 2>&1
tail -1 $OUT/bench.json | cut -c1-600
find $OUT -name "*.csv" | head -20
