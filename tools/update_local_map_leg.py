"""Timing of Tracking::UpdateLocalMap on the resident stores (capi.UpdateLocalMap.keyframes / .points) against the same two walks on the
host, under the protocol of the other store legs: ONE process on one GPU, host to host, p5 / median / p95 of --repeats after --warmup, the
forms alternating.
Shapes: 1 / 8 / 32 agents (one frame each, every agent its own keyframe store and map store); frames of 1 000 keypoints holding about 700
points of about 8 observations each; stores of 500 and of 2 000 keyframes of 1 000 to 1 900 entries; 80 local keyframes: the voted ones
and their nearest neighbours in slot order.
Forms:
  device_keyframes / device_points   each call on its own span, for all agents of the tick (capi.UpdateLocalMap.keyframes / .points: the
              span holds the Python wrapper's struct and array set-up too); the points call names each agent's 80 local keyframes
  host_numpy_one_agent  the table definitions of tests/local_map_scene.py (votes_table, local_points_table), ONE agent's walk
  host_cpp    tools/update_local_map_host_walk.cpp, compiled here with g++ -O2: std::map observation lists and pointer vectors, the two
              walks in the reference's order on its data structures, single thread, ONE agent's walk, in a process of its own (not alternated)
A tick of A agents costs A host walks on one host thread; the device call serves all A.
Every row carries same_results (device == numpy == C++ on votes, frame_bad, the list and frame_mp), the bytes up and down
(dvm_update_local_map_last_bytes) and the kernels' time with dvm_update_local_map_profile on.  Nothing is asserted on the times.
Usage: python tools/update_local_map_leg.py [--repeats 200] [--warmup 20] [--small] [--out profiles/update_local_map_leg.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dvm_slam_amd import capi  # noqa: E402
import keyframe_store_scene as kss  # noqa: E402
import local_map_scene as lms  # noqa: E402

LENS = (1000, 1130, 1260, 1390, 1520, 1650, 1780, 1900)
N_LOCAL = 80


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(p5_ms=round(float(np.percentile(a, 5)), 4), median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


class AgentMap:
    """One agent: n_kfs keyframes whose rows hold points of a sliding window of the map (a point is seen by about 8 consecutive
    keyframes), OBSERVED == MATCHES except for the last keyframe (queued: no observation yet); 2 % of the points bad."""

    def __init__(self, seed, n_kfs, frame_n, held, keyframes, small):
        rng = np.random.default_rng(seed)
        self.n_kfs = n_kfs
        self.lens = [LENS[int(i)] if not small else LENS[int(i)] // 10 for i in rng.integers(0, len(LENS), n_kfs)]
        per_kf = int(0.6 * np.mean(self.lens))
        self.n_points = max(per_kf * n_kfs // 8, per_kf * 2)
        step = self.n_points / n_kfs
        self.matches, self.observed = [], []
        for j, n in enumerate(self.lens):
            lo = int(j * step)
            window = (lo + np.arange(int(8 * step))) % self.n_points
            m = min(per_kf, len(window), n)
            row = np.full(n, -1, np.int32)
            row[rng.permutation(n)[:m]] = rng.choice(window, m, replace=False)
            self.matches.append(row)
            self.observed.append(row.copy() if j != n_kfs - 1 else np.full(n, -1, np.int32))
        self.bad = rng.random(self.n_points) < 0.02
        c = n_kfs // 2
        seen = np.unique(np.concatenate([r[r >= 0] for r in self.matches[c - 1:c + 2]]))
        frame = np.full(frame_n, -1, np.int32)
        frame[rng.permutation(frame_n)[:held]] = rng.choice(seen, held, replace=len(seen) < held)
        self.frame = frame
        self.kfs = capi.KeyframeStore(n_kfs, max(self.lens))
        self.points = capi.MapStore(self.n_points)
        rec = np.zeros(self.n_points, capi.LOCAL_POINT_DTYPE); rec["bad"] = self.bad
        self.points.update(np.arange(self.n_points, dtype=np.int32), rec)
        slots = np.arange(n_kfs, dtype=np.int32)
        for a in range(0, n_kfs, 250):
            b = min(a + 250, n_kfs)
            self.kfs.put(slots[a:b], [keyframes[n] for n in self.lens[a:b]])
            self.kfs.set_rows(capi.KFS_ROW_MATCHES, self.points, slots[a:b], self.matches[a:b])
            self.kfs.set_rows(capi.KFS_ROW_OBSERVED, self.points, slots[a:b], self.observed[a:b])

    def dump(self, path, local):
        w = [np.array([self.n_kfs], np.int32)]
        for n, o, m in zip(self.lens, self.observed, self.matches):
            w += [np.array([n], np.int32), o, m]
        w += [np.array([self.n_points], np.int32), self.bad.astype(np.int32), np.array([len(self.frame)], np.int32), self.frame,
              np.array([len(local)], np.int32), np.asarray(local, np.int32)]
        np.concatenate(w).astype(np.int32).tofile(path)

    def close(self):
        self.kfs.close(); self.points.close()


def local_of(votes):
    """The host's part, index work on the votes, in miniature: every voted keyframe, then -- as the neighbour / child / parent expansion
    does -- the keyframes nearest to them in slot order that are not included yet, up to N_LOCAL; in slot order."""
    voted = np.flatnonzero(votes > 0)
    if len(voted) == 0:
        return voted.astype(np.int32)
    if len(voted) >= N_LOCAL:
        return np.sort(voted[np.argsort(-votes[voted], kind="stable")[:N_LOCAL]]).astype(np.int32)
    rest = np.setdiff1d(np.arange(len(votes)), voted)
    near = rest[np.argsort(np.abs(rest - int(np.median(voted))), kind="stable")[:N_LOCAL - len(voted)]]
    return np.sort(np.concatenate([voted, near])).astype(np.int32)


def run_shape(agents, n_kfs, exe, repeats, warmup, small):
    keyframes = {n // 10 if small else n: kss.keyframe(n, n // 10 if small else n) for n in LENS}
    maps = [AgentMap(100 * n_kfs + a, n_kfs, 1000 if not small else 100, 700 if not small else 70, keyframes, small) for a in range(agents)]
    ulm = capi.UpdateLocalMap()
    ulm.reserve(agents, len(maps[0].frame), N_LOCAL, max(m.n_points for m in maps), n_kfs, max(max(m.lens) for m in maps))
    res = {}

    def device():
        k = ulm.keyframes([dict(kfs=m.kfs, points=m.points, mp_slot=m.frame) for m in maps])
        res["up_k"], res["down_k"] = ulm.last_bytes(); res["ms_k"] = ulm.last_ms()
        local = [local_of(r["votes"]) for r in k]
        p = ulm.points([dict(kfs=m.kfs, points=m.points, kf_slot=l, mp_slot=np.where(r["frame_bad"] != 0, -1, m.frame).astype(np.int32))
                        for m, l, r in zip(maps, local, k)])
        res["up_p"], res["down_p"] = ulm.last_bytes(); res["ms_p"] = ulm.last_ms()
        res["device"] = (k, local, p)

    def host_numpy(all_agents=False):
        out = []
        for m in maps if all_agents else maps[:1]:
            votes, frame_bad = lms.votes_table(m.frame, m.bad, dict(enumerate(m.observed)), m.n_kfs)
            local = local_of(votes)
            out.append((votes, frame_bad, local, lms.local_points_table(local, m.matches, m.bad, m.frame)))
        res["numpy"] = out
    ulm.profile(True)
    device(); host_numpy(all_agents=True)
    kernel_ms = dict(keyframes=round(res["ms_k"], 4), points=round(res["ms_p"], 4))
    ulm.profile(False)
    k, local, p = res["device"]
    same = True
    for b, (votes, frame_bad, loc, (local_slot, frame_mp, n_out)) in enumerate(res["numpy"]):
        same &= np.array_equal(k[b]["votes"], votes) and np.array_equal(k[b]["frame_bad"], frame_bad) and np.array_equal(local[b], loc)
        same &= np.array_equal(p[b]["local_slot"], local_slot) and np.array_equal(p[b]["frame_mp"], frame_mp) and p[b]["n_outside"] == n_out
    # the C++ walk of agent 0
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.i32")
        maps[0].dump(path, local[0])
        cpp = json.loads(subprocess.run([exe, path, str(repeats), str(warmup)], capture_output=True, text=True, check=True).stdout)
    h = 0
    for s in p[0]["local_slot"]:
        h = (h * 1000003 + int(s)) % 2147483647
    same &= cpp["votes_sum"] == int(k[0]["votes"].sum()) and cpp["voted_keyframes"] == int((k[0]["votes"] > 0).sum())
    same &= cpp["n_local"] == p[0]["n_local"] and cpp["local_hash"] == h and cpp["frame_bad"] == int(k[0]["frame_bad"].sum())
    # the spans: each device call on its own (the points call on the lists the first pass left), and the numpy form
    kf_frames = [dict(kfs=m.kfs, points=m.points, mp_slot=m.frame) for m in maps]
    pt_frames = [dict(kfs=m.kfs, points=m.points, kf_slot=l, mp_slot=np.where(r["frame_bad"] != 0, -1, m.frame).astype(np.int32))
                 for m, l, r in zip(maps, local, k)]
    calls = dict(device_keyframes=lambda: ulm.keyframes(kf_frames), device_points=lambda: ulm.points(pt_frames), host_numpy_one_agent=host_numpy)
    times = {k_: [] for k_ in calls}
    order = list(calls.items())
    for it in range(warmup + repeats):
        for name, f in order[it % 3:] + order[:it % 3]:
            t0 = time.perf_counter(); f(); t1 = time.perf_counter()
            if it >= warmup:
                times[name].append(t1 - t0)
    row = dict(leg="update_local_map", agents=agents, keyframes=n_kfs, map_points=maps[0].n_points, frame_keypoints=len(maps[0].frame),
               held=int((maps[0].frame >= 0).sum()), row_entries=int(sum(maps[0].lens)), local_keyframes=[len(l) for l in local][:4],
               n_local=[r["n_local"] for r in p][:4], n_outside=[r["n_outside"] for r in p][:4], same_results=bool(same),
               bytes_up=dict(keyframes=res["up_k"], points=res["up_p"]), bytes_down=dict(keyframes=res["down_k"], points=res["down_p"]),
               call_span={k_: stats(v) for k_, v in times.items()}, kernel_ms=kernel_ms,
               host_cpp_one_agent=dict(votes=cpp["votes"], points=cpp["points"], n=cpp["n"],
                                       note="a process of its own, run once before the alternating spans, not alternated with them"))
    ulm.close()
    for m in maps:
        m.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--shapes", default="1x500,8x500,32x500,1x2000,8x2000,32x2000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_local_map_leg.json"))
    a = ap.parse_args()
    capi.lib()
    os.makedirs(os.path.join(ROOT, "tools", "bin"), exist_ok=True)
    exe = os.path.join(ROOT, "tools", "bin", "update_local_map_host_walk")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "update_local_map_host_walk.cpp")])
    lines = []
    for shape in a.shapes.split(","):
        agents, n_kfs = (int(x) for x in shape.split("x"))
        if a.small:
            n_kfs = max(n_kfs // 10, 20)
        lines.append(json.dumps(run_shape(agents, n_kfs, exe, a.repeats, a.warmup, a.small)))
        print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not all(json.loads(l)["same_results"] for l in lines):
        sys.exit("a row whose forms differ")


if __name__ == "__main__":
    main()
