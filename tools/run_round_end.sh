# tools/run_round_end.sh OUTDIR -- GPU tests, the --full bench line, smoke, and rocprofv3 kernel stats of a --full run, into OUTDIR
set -x
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:?usage: tools/run_round_end.sh OUTDIR}" && cd "$1" && pwd)
cd "$R"
python -m pytest tests -m gpu -x -q 2>&1 | tail -4
python bench.py --full 2>&1 | tail -1 > $O/bench_k.json
cut -c1-600 $O/bench_k.json
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_k
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_k -- python $R/bench.py --full --steps 10 --warmup 2 --cpu-seconds 0 > $O/prof_k.log 2>&1
find $O/prof_k -name "*kernel_stats.csv" | head
