"""tools/fold_profiles_pyr_direct.py OUT_DIR RUNS [name=lib ...] -- folds what tools/run_profiles_pyr_direct.sh left in OUT_DIR into
OUT_DIR/pd_ab.json: the benchmark's values with the acceptance test, every resize launch's time alone, the counters per resize launch."""
import collections
import csv
import glob
import json
import os
import statistics
import sys

o, runs = sys.argv[1], int(sys.argv[2])
variants = [v.split("=")[0] for v in sys.argv[3:]]
out = {}


def value(name):
    p = f"{o}/bench_{name}.json"
    return json.load(open(p))["value"] if os.path.exists(p) and os.path.getsize(p) else None


par = [value(f"parent_{i}") for i in range(1, runs + 1)]
tre = [value(f"tree_{i}") for i in range(1, runs + 1)]
if all(v is not None for v in par + tre):
    spread = max(par) - min(par)
    gain = statistics.median(tre) - statistics.median(par)
    out["bench"] = {
        "command": "python bench.py --gpus 1 --steps 20 --warmup 5", "unit": "frames/s", "parent": par, "tree": tre,
        "parent_median": statistics.median(par), "tree_median": statistics.median(tre), "parent_spread": spread,
        "median_gain": gain, "median_gain_percent": 100 * gain / statistics.median(par),
        "every_tree_run_above_every_parent_run": min(tre) > max(par), "gain_at_least_3x_parent_spread": gain >= 3 * spread,
        "tree_DVM_PYR_DIRECT_0": value("tree_direct0"), "tree_DVM_PYR_DIRECT_1": value("tree_direct1"),
        "variants": {v: value(v) for v in variants}}
    out["bench"]["accepted"] = out["bench"]["every_tree_run_above_every_parent_run"] and out["bench"]["gain_at_least_3x_parent_spread"]

alone = {}
for p in sorted(glob.glob(f"{o}/pd_*_resize_levels.csv")):
    name = os.path.basename(p)[3:-len("_resize_levels.csv")]
    rows = list(csv.DictReader(open(p)))
    alone[name] = {"launches": [{"level": int(r["level"]), "kernel": r["kernel"], "avg_us": float(r["avg_us"]), "min_us": float(r["min_us"])} for r in rows],
                   "sum_avg_us": round(sum(float(r["avg_us"]) for r in rows), 2)}
out["resize_launches_us"] = alone

stats = {}
for p in sorted(glob.glob(f"{o}/pd_*_kernel_stats.csv")):
    name = os.path.basename(p)[3:-len("_kernel_stats.csv")]
    stats[name] = {r["Name"].split("(")[0].split("::")[-1]: {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
                   for r in csv.DictReader(open(p)) if "dvm::" in r["Name"]}
out["kernel_stats_avg_us"] = stats

pmc = {}
for side in ("parent", "tree"):
    for name in ("sq_counters", "FETCH_SIZE", "WRITE_SIZE"):
        p = f"{o}/pd_pmc_{side}_{name}.csv"
        if not os.path.exists(p):
            continue
        agg, level, last = collections.defaultdict(lambda: collections.defaultdict(list)), 0, None
        for r in sorted(csv.DictReader(open(p)), key=lambda r: int(r["Dispatch_Id"])):   # (one lane, one stream: dispatch order = launch order)
            k = r["Kernel_Name"].split("(")[0].split("::")[-1]
            if "k_pyr_level0" not in k and "k_pyr_resize" not in k:
                continue
            if r["Dispatch_Id"] != last:   # (one row per counter and dispatch)
                last, level = r["Dispatch_Id"], 0 if "k_pyr_level0" in k else level + 1
            agg[(level, k)][r["Counter_Name"]].append(float(r["Counter_Value"]))
        for (l, k), c in sorted(agg.items()):
            pmc.setdefault(side, {}).setdefault(f"level {l} {k}", {}).update({a: round(sum(b) / len(b)) for a, b in c.items()})
for side, launches in pmc.items():
    tot = collections.Counter()
    for k, c in launches.items():
        if "k_pyr_resize" in k:
            tot.update(c)
    launches["resize launches summed"] = dict(tot)
out["counters_per_launch"] = pmc
json.dump(out, open(f"{o}/pd_ab.json", "w"), indent=1)
print(json.dumps({k: out[k] for k in ("bench",) if k in out}, indent=1))
for n, a in alone.items():
    print(n, "resize launches, us:", [l["avg_us"] for l in a["launches"]], "sum", a["sum_avg_us"])
for side, launches in pmc.items():
    print(side, launches.get("resize launches summed"))
