// tools/update_local_map_host_walk.cpp -- the host side of tools/update_local_map_leg.py: Tracking::UpdateLocalMap's two walks on a pointer
// graph, single thread, with the data structures and the order of work of the reference (src/Tracking.cc:3117-3181) -- an ordered map of
// observations copied per point, an ordered map as the vote table, pointer vectors copied per keyframe, a per-frame mark on the point.  The leg dumps a
// scene as int32 words and reads back one JSON line: the times of both walks and what they computed, which the leg holds against the
// device's results.
//   file: n_kfs_total, then per keyframe its length and its OBSERVED row and its MATCHES row; n_points, bad[n_points]; n frame entries,
//         the frame's slots; n_local_kfs, the local keyframes in the loop's visiting order
// Usage: update_local_map_host_walk FILE REPEATS WARMUP
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

struct Kf;
using ObsList = std::map<Kf*, std::tuple<int, int>>;   // keyframe -> (left index, right index), ordered by address
struct Pt {
  ObsList obs;
  bool bad = false;
  long seen_in_frame = -1;                             // the per-frame mark of the local-point walk
  int slot = 0;
  ObsList observations() const { return obs; }         // a copy, as a getter behind a mutex hands one out
};
struct Kf {
  std::vector<Pt*> held;
  int slot = 0;
  std::vector<Pt*> matches() const { return held; }    // a copy, likewise
};

static double pct(std::vector<double> v, double p) {
  std::sort(v.begin(), v.end());
  const double x = p * (double)(v.size() - 1);
  const size_t i = (size_t)x;
  return i + 1 < v.size() ? v[i] + (x - (double)i) * (v[i + 1] - v[i]) : v[i];
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<int32_t> w((size_t)bytes / 4);
  if (std::fread(w.data(), 4, w.size(), f) != w.size()) return 2;
  std::fclose(f);
  const int repeats = std::atoi(argv[2]), warmup = std::atoi(argv[3]);
  size_t at = 0;
  const int n_kfs = w[at++];
  std::vector<Kf> kfs((size_t)n_kfs);
  std::vector<std::vector<int32_t>> observed((size_t)n_kfs), matches((size_t)n_kfs);
  for (int j = 0; j < n_kfs; j++) {
    const int len = w[at++];
    observed[(size_t)j].assign(w.begin() + (long)at, w.begin() + (long)at + len); at += (size_t)len;
    matches[(size_t)j].assign(w.begin() + (long)at, w.begin() + (long)at + len); at += (size_t)len;
  }
  const int n_points = w[at++];
  std::vector<Pt> points((size_t)n_points);
  for (int p = 0; p < n_points; p++) { points[(size_t)p].bad = w[at++] != 0; points[(size_t)p].slot = p; }
  for (int j = 0; j < n_kfs; j++) {
    Kf& kf = kfs[(size_t)j];
    kf.slot = j;
    kf.held.assign(matches[(size_t)j].size(), nullptr);
    for (size_t kp = 0; kp < matches[(size_t)j].size(); kp++) {
      if (matches[(size_t)j][kp] >= 0) kf.held[kp] = &points[(size_t)matches[(size_t)j][kp]];
      if (observed[(size_t)j][kp] >= 0) points[(size_t)observed[(size_t)j][kp]].obs[&kf] = std::make_tuple((int)kp, -1);
    }
  }
  const int n = w[at++];
  std::vector<Pt*> frame0((size_t)n, nullptr);
  for (int i = 0; i < n; i++) { const int32_t s = w[at++]; if (s >= 0) frame0[(size_t)i] = &points[(size_t)s]; }
  const int n_local = w[at++];
  std::vector<Kf*> visit;                                            // the local keyframes in visiting order
  for (int k = 0; k < n_local; k++) visit.push_back(&kfs[(size_t)w[at + (size_t)k]]);

  std::vector<double> t_votes, t_points;
  long long votes_sum = 0, votes_kfs = 0, local_points = 0, local_hash = 0, cleared = 0;
  for (int it = 0; it < warmup + repeats; it++) {
    std::vector<Pt*> frame = frame0;                                 // the frame's own list: bad entries are cleared in it
    const long frame_id = it + 1;
    const auto t0 = std::chrono::steady_clock::now();
    // the votes: every live point of the frame gives one to each keyframe of its (copied) observation list
    std::map<Kf*, int> tally;
    for (Pt*& p : frame) {
      if (p == nullptr) continue;
      if (p->bad) { p = nullptr; continue; }
      const ObsList seen_by = p->observations();
      for (const auto& o : seen_by) ++tally[o.first];
    }
    const auto t1 = std::chrono::steady_clock::now();
    // the local points: the keyframes' (copied) match lists in visiting order, every live point once, marked with the frame's id
    std::vector<Pt*> local;
    for (Kf* kf : visit) {
      const std::vector<Pt*> held = kf->matches();
      for (Pt* p : held) {
        if (p == nullptr || p->seen_in_frame == frame_id || p->bad) continue;
        p->seen_in_frame = frame_id;
        local.push_back(p);
      }
    }
    const auto t2 = std::chrono::steady_clock::now();
    if (it >= warmup) {
      t_votes.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
      t_points.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    votes_sum = votes_kfs = local_hash = cleared = 0;
    for (const auto& kv : tally) { votes_sum += kv.second; votes_kfs++; }
    local_points = (long long)local.size();
    for (const Pt* p : local) local_hash = (local_hash * 1000003 + p->slot) % 2147483647;
    for (int i = 0; i < n; i++) cleared += frame0[(size_t)i] && !frame[(size_t)i];
  }
  std::printf("{\"votes\": {\"p5_ms\": %.4f, \"median_ms\": %.4f, \"p95_ms\": %.4f}, \"points\": {\"p5_ms\": %.4f, \"median_ms\": %.4f, \"p95_ms\": %.4f}, "
              "\"votes_sum\": %lld, \"voted_keyframes\": %lld, \"n_local\": %lld, \"local_hash\": %lld, \"frame_bad\": %lld, \"n\": %d}\n",
              pct(t_votes, 0.05), pct(t_votes, 0.5), pct(t_votes, 0.95), pct(t_points, 0.05), pct(t_points, 0.5), pct(t_points, 0.95), votes_sum, votes_kfs,
              local_points, local_hash, cleared, repeats);
  return 0;
}
