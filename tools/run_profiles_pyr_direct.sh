# tools/run_profiles_pyr_direct.sh PARENT_LIB [OUT_DIR] -- rocprofv3 evidence and the A/B benchmark for k_pyr_resize_direct (the pyramid
# resize that loads its source bytes straight from global memory); run on the MI355X, output under OUT_DIR (default bench_out/prof_pd;
# the pd_* files are copied to profiles/).  PARENT_LIB = a build of the parent commit; both libraries are selected through DVM_HIP_LIB.
#   1. --kernel-trace --stats of the timed region of bench.py, two lanes: parent and tree     -> pd_parent_kernel_stats.csv, pd_tree_kernel_stats.csv
#   2. the same on ONE lane with everything on one stream (DVM_SERIAL=1): a kernel's duration is its time alone on the chip
#                                        -> pd_alone_{parent,tree}_kernel_stats.csv, and per resize launch (= per level) pd_alone_{parent,tree}_resize_levels.csv
#   3. separate --pmc passes, no tracing: SQ counters | FETCH_SIZE | WRITE_SIZE of a short one-lane run, dvm kernels only, both sides
#                                                                                              -> pd_pmc_{parent,tree}_*.csv
#   4. python bench.py --gpus 1 --steps 20 --warmup 5 in fresh processes, parent and tree alternating, PD_RUNS (default 3) a side, then the
#      tree's library with DVM_PYR_DIRECT=0 / 1                                                -> pd_ab.json (with the figures of 2 and 3)
# PD_VARIANTS="name=lib ..." (optional): measurement builds of the tree (make EXTRA=-DDVM_PYR_NS=n) that get item 2 and one bench run each.
# PD_PARTS="stats pmc bench" (default: all three): the parts to run, for a session that has to split the work; the fold reads what is there.
# Every GPU step runs under its own timeout; the first failure ends the script.
set -u
PARTS=${PD_PARTS:-stats pmc bench}
want() { case " $PARTS " in *" $1 "*) return 0;; esac; return 1; }
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?path of a libdvmslam_hip.so built from the parent commit}
TREE=$R/dvm_slam_amd/lib/libdvmslam_hip.so
O=${2:-$R/bench_out/prof_pd}
RUNS=${PD_RUNS:-3}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
FOLD='import csv, sys
rows = [r for r in csv.DictReader(open(sys.argv[1])) if "dvm::" in r["Kernel_Name"]]
keep = ["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value", "Grid_Size", "Workgroup_Size", "LDS_Block_Size", "VGPR_Count", "SGPR_Count"]
keep = [k for k in keep if rows and k in rows[0]]
w = csv.DictWriter(open(sys.argv[2], "w"), keep); w.writeheader()
for r in rows: w.writerow({k: r[k] for k in keep})'
# per resize launch: a queue's dispatches in order, the resizes behind each k_pyr_level0 are levels 1, 2, ... of that launch group
LEVELS='import collections, csv, sys
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: (r.get("Queue_Id", ""), int(r["Start_Timestamp"])))
g, level, queue = collections.defaultdict(list), 0, None
for r in rows:
    if r.get("Queue_Id", "") != queue: queue, level = r.get("Queue_Id", ""), 0
    if "k_pyr_level0" in r["Kernel_Name"]: level = 0
    elif "k_pyr_resize" in r["Kernel_Name"]:
        level += 1
        g[(level, r["Kernel_Name"].split("(")[0].split("::")[-1])].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
w = csv.writer(open(sys.argv[2], "w")); w.writerow(["level", "kernel", "calls", "avg_us", "min_us"])
for (l, k), d in sorted(g.items()): w.writerow([l, k, len(d), round(sum(d) / len(d) / 1e3, 2), round(min(d) / 1e3, 2)])'
ARGS="--steps 3 --warmup 1 --chunks-per-step 8 --no-ba --no-pcie --no-exclusive --no-legs --no-config-legs --cpu-seconds 0"
SHORT="--steps 1 --warmup 1 --chunks-per-step 2 --no-ba --no-pcie --no-exclusive --no-legs --no-config-legs --cpu-seconds 0 --lanes 1"
stats() {   # name, then environment assignments, "--", then bench.py arguments
  local name=$1; shift
  local envs=(); while [ "$1" != "--" ]; do envs+=("$1"); shift; done; shift
  rm -rf /tmp/pd_$name
  env "${envs[@]}" timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pd_$name -- python $R/bench.py "$@" > $O/$name.log 2>&1 || { echo "$name failed"; tail -5 $O/$name.log; exit 1; }
  cp "$(find /tmp/pd_$name -name '*kernel_stats.csv' | head -1)" $O/pd_${name}_kernel_stats.csv
  python -c "$LEVELS" "$(find /tmp/pd_$name -name '*kernel_trace.csv' | head -1)" $O/pd_${name}_resize_levels.csv || exit 1
  echo "stats $name done"
}
if want stats; then
  stats parent DVM_HIP_LIB=$PARENT -- $ARGS
  stats tree DVM_HIP_LIB=$TREE -- $ARGS
  stats alone_parent DVM_HIP_LIB=$PARENT DVM_SERIAL=1 -- $ARGS --lanes 1
  stats alone_tree DVM_HIP_LIB=$TREE DVM_SERIAL=1 -- $ARGS --lanes 1
  for v in ${PD_VARIANTS:-}; do stats alone_${v%%=*} DVM_HIP_LIB=${v#*=} DVM_SERIAL=1 -- $ARGS --lanes 1; done
fi
pmc() {   # side, library, name, counters...
  local side=$1 lib=$2 name=$3; shift 3
  rm -rf /tmp/pd_pmc_${side}_$name
  DVM_HIP_LIB=$lib DVM_SERIAL=1 timeout -k 10 240 rocprofv3 --pmc "$@" --output-format csv -d /tmp/pd_pmc_${side}_$name -- python $R/bench.py $SHORT > $O/pmc_${side}_$name.log 2>&1 || { echo "pmc $side $name failed"; tail -5 $O/pmc_${side}_$name.log; exit 1; }
  python -c "$FOLD" "$(find /tmp/pd_pmc_${side}_$name -name '*counter_collection.csv' | head -1)" $O/pd_pmc_${side}_$name.csv || exit 1
  echo "pmc $side $name done"
}
for side in parent tree; do
  want pmc || break
  lib=$PARENT; [ $side = tree ] && lib=$TREE
  pmc $side $lib sq_counters SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_WAVES
  pmc $side $lib FETCH_SIZE FETCH_SIZE
  pmc $side $lib WRITE_SIZE WRITE_SIZE
done
bench() {   # name, then environment assignments: one fresh process, its JSON result line -> $O/bench_<name>.json
  local name=$1; shift
  env "$@" timeout -k 10 400 python $R/bench.py --gpus 1 --steps 20 --warmup 5 > $O/bench_$name.log 2>&1 || { echo "bench $name failed"; tail -5 $O/bench_$name.log; exit 1; }
  grep '^{' $O/bench_$name.log | tail -1 > $O/bench_$name.json
  python -c "import json, sys; print('bench $name value', json.load(open(sys.argv[1]))['value'])" $O/bench_$name.json || exit 1
}
cd $R
if want bench; then
  for i in $(seq 1 $RUNS); do
    bench parent_$i DVM_HIP_LIB=$PARENT
    bench tree_$i DVM_HIP_LIB=$TREE
  done
  bench tree_direct0 DVM_HIP_LIB=$TREE DVM_PYR_DIRECT=0
  bench tree_direct1 DVM_HIP_LIB=$TREE DVM_PYR_DIRECT=1
  for v in ${PD_VARIANTS:-}; do bench ${v%%=*} DVM_HIP_LIB=${v#*=}; done
fi
python $R/tools/fold_profiles_pyr_direct.py $O $RUNS ${PD_VARIANTS:-} || exit 1
