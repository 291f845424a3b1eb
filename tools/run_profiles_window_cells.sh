# tools/run_profiles_window_cells.sh PARENT_LIB [OUT_DIR] -- rocprofv3 evidence for the window scan over the cell rectangle (window_scan,
# FrameView::cell_start) and the one-launch dvm_orb_copy_result; run on the MI355X, output under OUT_DIR (default bench_out/prof_wc; the
# wc_*.csv are copied to profiles/).  PARENT_LIB = a build of the parent commit; both libraries are selected through DVM_HIP_LIB.
#   1. --kernel-trace --stats of the timed region of bench.py, two lanes: parent and tree     -> wc_parent_kernel_stats.csv, wc_tree_kernel_stats.csv
#   2. the same on ONE lane with everything on one stream (DVM_SERIAL=1): a kernel's duration is its time alone on the chip
#                                                                                              -> wc_alone_parent_kernel_stats.csv, wc_alone_tree_kernel_stats.csv
#   3. separate --pmc passes, no tracing: SQ counters | FETCH_SIZE | WRITE_SIZE of a short one-lane run, dvm kernels only, both sides
#                                                                                              -> wc_pmc_{parent,tree}_*.csv
# Every GPU step runs under its own timeout; the first failure ends the script.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?path of a libdvmslam_hip.so built from the parent commit}
TREE=$R/dvm_slam_amd/lib/libdvmslam_hip.so
O=${2:-$R/bench_out/prof_wc}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
FOLD='import csv, sys
rows = [r for r in csv.DictReader(open(sys.argv[1])) if "dvm::" in r["Kernel_Name"]]
keep = ["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value", "Grid_Size", "Workgroup_Size", "LDS_Block_Size", "VGPR_Count", "SGPR_Count"]
keep = [k for k in keep if rows and k in rows[0]]
w = csv.DictWriter(open(sys.argv[2], "w"), keep); w.writeheader()
for r in rows: w.writerow({k: r[k] for k in keep})'
ARGS="--steps 3 --warmup 1 --chunks-per-step 8 --no-ba --no-pcie --no-exclusive --no-legs --no-config-legs --cpu-seconds 0"
SHORT="--steps 1 --warmup 1 --chunks-per-step 2 --no-ba --no-pcie --no-exclusive --no-legs --no-config-legs --cpu-seconds 0 --lanes 1"
stats() {   # name, then environment assignments, "--", then bench.py arguments
  local name=$1; shift
  local envs=(); while [ "$1" != "--" ]; do envs+=("$1"); shift; done; shift
  rm -rf /tmp/wc_$name
  env "${envs[@]}" timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/wc_$name -- python $R/bench.py "$@" > $O/$name.log 2>&1 || { echo "$name failed"; tail -5 $O/$name.log; exit 1; }
  cp "$(find /tmp/wc_$name -name '*kernel_stats.csv' | head -1)" $O/wc_${name}_kernel_stats.csv
}
stats parent DVM_HIP_LIB=$PARENT -- $ARGS
stats tree DVM_HIP_LIB=$TREE -- $ARGS
stats alone_parent DVM_HIP_LIB=$PARENT DVM_SERIAL=1 -- $ARGS --lanes 1
stats alone_tree DVM_HIP_LIB=$TREE DVM_SERIAL=1 -- $ARGS --lanes 1
pmc() {   # side, library, name, counters...
  local side=$1 lib=$2 name=$3; shift 3
  rm -rf /tmp/wc_pmc_${side}_$name
  DVM_HIP_LIB=$lib DVM_SERIAL=1 timeout -k 10 240 rocprofv3 --pmc "$@" --output-format csv -d /tmp/wc_pmc_${side}_$name -- python $R/bench.py $SHORT > $O/pmc_${side}_$name.log 2>&1 || { echo "pmc $side $name failed"; tail -5 $O/pmc_${side}_$name.log; exit 1; }
  python -c "$FOLD" "$(find /tmp/wc_pmc_${side}_$name -name '*counter_collection.csv' | head -1)" $O/wc_pmc_${side}_$name.csv
}
for side in parent tree; do
  lib=$PARENT; [ $side = tree ] && lib=$TREE
  pmc $side $lib sq_counters SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_WAVES
  pmc $side $lib FETCH_SIZE FETCH_SIZE
  pmc $side $lib WRITE_SIZE WRITE_SIZE
done
python - $O <<'EOF'
import collections, csv, sys
o = sys.argv[1]
for name in ("parent", "tree", "alone_parent", "alone_tree"):
    for r in csv.DictReader(open(f"{o}/wc_{name}_kernel_stats.csv")):
        if any(k in r["Name"] for k in ("k_match_window", "k_frame_build", "k_copy_result", "copyBuffer")):
            print(name, r["Name"].split("(")[0], r["Calls"], "avg us", round(float(r["AverageNs"]) / 1e3, 1))
for side in ("parent", "tree"):
    for name in ("sq_counters", "FETCH_SIZE", "WRITE_SIZE"):
        agg = collections.defaultdict(lambda: collections.defaultdict(list))
        for r in csv.DictReader(open(f"{o}/wc_pmc_{side}_{name}.csv")):
            if "k_match_window" in r["Kernel_Name"] or "k_frame_build" in r["Kernel_Name"]:
                agg[r["Kernel_Name"].split("(")[0]][r["Counter_Name"]].append(float(r["Counter_Value"]))
        for k, c in agg.items():
            print(side, name, k, {a: round(sum(b) / len(b)) for a, b in c.items()})
EOF
