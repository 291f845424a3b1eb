# tools/run_profiles_patch_blur.sh PARENT_LIB [OUT_DIR] -- rocprofv3 evidence for the descriptor kernel that blurs its own patches
# (k_orient_desc_blur, DVM_PATCH_BLUR); run on the MI355X, output under OUT_DIR (default bench_out/prof_pb; the pb_*.csv are copied to profiles/)
#   1. --kernel-trace --stats of the timed region of bench.py: the parent's library (PARENT_LIB = a build of the parent commit,
#      selected through DVM_HIP_LIB) and this tree's                                          -> pb_parent_kernel_stats.csv, pb_branch_kernel_stats.csv
#   2. the same on ONE lane with everything on one stream (DVM_SERIAL=1), so that a kernel's duration is its time alone on the
#      chip: blurred-pyramid pair (DVM_PATCH_BLUR=0) and the fused kernel                     -> pb_alone_pair_kernel_stats.csv, pb_alone_fused_kernel_stats.csv
#   3. separate --pmc passes, no tracing: SQ counters | FETCH_SIZE | WRITE_SIZE of a short one-lane run, dvm kernels only -> pb_pmc_*.csv
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?path of a libdvmslam_hip.so built from the parent commit}
O=${2:-$R/bench_out/prof_pb}
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
  rm -rf /tmp/pb_$name
  env "${envs[@]}" timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pb_$name -- python $R/bench.py "$@" > $O/$name.log 2>&1 || { echo "$name failed"; tail -5 $O/$name.log; exit 1; }
  cp "$(find /tmp/pb_$name -name '*kernel_stats.csv' | head -1)" $O/pb_${name}_kernel_stats.csv
}
stats parent DVM_HIP_LIB=$PARENT -- $ARGS
stats branch DVM_PATCH_BLUR=1 -- $ARGS
stats alone_pair DVM_PATCH_BLUR=0 DVM_SERIAL=1 -- $ARGS --lanes 1
stats alone_fused DVM_PATCH_BLUR=1 DVM_SERIAL=1 -- $ARGS --lanes 1
pmc() {   # name, counters...
  local name=$1; shift
  rm -rf /tmp/pb_pmc_$name
  DVM_PATCH_BLUR=1 DVM_SERIAL=1 timeout -k 10 240 rocprofv3 --pmc "$@" --output-format csv -d /tmp/pb_pmc_$name -- python $R/bench.py $SHORT > $O/pmc_$name.log 2>&1 || { echo "pmc $name failed"; tail -5 $O/pmc_$name.log; exit 1; }
  python -c "$FOLD" "$(find /tmp/pb_pmc_$name -name '*counter_collection.csv' | head -1)" $O/pb_pmc_$name.csv
}
pmc sq_counters SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_WAVES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE
pmc FETCH_SIZE FETCH_SIZE
pmc WRITE_SIZE WRITE_SIZE
python - $O <<'EOF'
import collections, csv, sys
o = sys.argv[1]
for name in ("parent", "branch", "alone_pair", "alone_fused"):
    for r in csv.DictReader(open(f"{o}/pb_{name}_kernel_stats.csv")):
        if any(k in r["Name"] for k in ("k_orient_desc", "k_blur7")):
            print(name, r["Name"].split("(")[0], r["Calls"], "avg us", round(float(r["AverageNs"]) / 1e3, 1))
for name in ("sq_counters", "FETCH_SIZE", "WRITE_SIZE"):
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f"{o}/pb_pmc_{name}.csv")):
        if "k_orient_desc" in r["Kernel_Name"]:
            agg[r["Kernel_Name"].split("(")[0]][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k, c in agg.items():
        print(name, k, {a: round(sum(b) / len(b)) for a, b in c.items()})
EOF
