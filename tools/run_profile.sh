# rocprofv3 kernel stats of the timed region only (no BA / PCIe / exclusive legs): averages comparable with bench.py's HIP events
# (--full: the roofline's live k_fast_cells events); tools/run_profile.sh OUTDIR
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:?usage: tools/run_profile.sh OUTDIR}" && cd "$1" && pwd)
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_l
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_l -- python $R/bench.py --full --steps 20 --warmup 2 --cpu-seconds 0 --no-ba --no-pcie --no-exclusive > $O/prof_l.log 2>&1
tail -1 $O/prof_l.log | cut -c1-300
find $O/prof_l -name "*kernel_stats.csv" | head -1 | xargs head -12 | cut -c1-120
