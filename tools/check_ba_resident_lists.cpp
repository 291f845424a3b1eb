// tools/check_ba_resident_lists.cpp -- the host lists of dvm_ba_resident_optimize's prepare step (dvm_slam_amd/csrc/ba_resident_lists.h)
// against a brute-force restatement: a point's edges are exactly the edges that name it, ascending (the caller's order); pe_start is
// monotone from 0 to E; an edge outside the window is refused; ref_edge passes only where it is an edge of its point, -1 only on a point
// without edges.  Windows at E and L of 0, 1, 63, 64, 65 and 257, with points without edges and a point seen twice by one camera.  Plain
// g++, no HIP header (tests/test_ba_resident_lists.py builds it, also with sanitizers).
#include <cstdio>
#include <random>
#include <vector>

#include "../dvm_slam_amd/csrc/ba_resident_lists.h"

using namespace dvm;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void window(int P, int L, int E, unsigned seed) {
  std::mt19937 rng(seed);
  std::vector<dvm_ba_obs> obs((size_t)E);
  const int used = L > 2 ? L - 2 : L;                  // the last two points have no edge
  for (int e = 0; e < E; e++) obs[(size_t)e] = dvm_ba_obs{(int32_t)(rng() % (unsigned)P), (int32_t)(rng() % (unsigned)used), (int32_t)(rng() % 100u)};
  if (E >= 2) obs[(size_t)E - 1] = dvm_ba_obs{obs[0].pose, obs[0].point, obs[0].kp + 1};     // a point seen twice by one camera
  ResidentLists r;
  EXPECT(resident_lists_build(obs.data(), P, L, E, r) == 0);
  EXPECT((int)r.pe_start.size() == L + 1 && (int)r.pe_edges.size() == E);
  EXPECT(r.pe_start[0] == 0 && r.pe_start[(size_t)L] == E);
  std::vector<int32_t> ref((size_t)L, -1);
  for (int l = 0; l < L; l++) {
    std::vector<int32_t> mine;
    for (int e = 0; e < E; e++) if (obs[(size_t)e].point == l) mine.push_back(e);
    EXPECT(r.pe_start[(size_t)l + 1] - r.pe_start[(size_t)l] == (int)mine.size());
    for (size_t i = 0; i < mine.size() && r.pe_start[(size_t)l] + (int)i < E; i++) EXPECT(r.pe_edges[(size_t)r.pe_start[(size_t)l] + i] == mine[i]);
    if (!mine.empty()) ref[(size_t)l] = mine[rng() % mine.size()];
  }
  int at = -1;
  EXPECT(resident_ref_check(obs.data(), L, E, r, ref.data(), &at) == 0);
  for (int l = 0; l < L; l++) {
    const int32_t keep = ref[(size_t)l];
    const bool has = keep >= 0;
    ref[(size_t)l] = E;                                 // out of range
    EXPECT(resident_ref_check(obs.data(), L, E, r, ref.data(), &at) == 1 && at == l);
    ref[(size_t)l] = -2;
    EXPECT(resident_ref_check(obs.data(), L, E, r, ref.data(), &at) == 1 && at == l);
    if (has) {
      ref[(size_t)l] = -1;                              // -1 on a point that has edges
      EXPECT(resident_ref_check(obs.data(), L, E, r, ref.data(), &at) == 3 && at == l);
    }
    for (int e = 0; e < E; e++)
      if (obs[(size_t)e].point != l) {                  // an edge of another point
        ref[(size_t)l] = e;
        EXPECT(resident_ref_check(obs.data(), L, E, r, ref.data(), &at) == 2 && at == l);
        break;
      }
    ref[(size_t)l] = keep;
    if (l >= 8 && l < L - 3) l += L / 7;                // (every point of a small window, a sample of a large one)
  }
  if (E > 0) {                                           // refusals: each index one past its range, and negative
    const dvm_ba_obs keep = obs[(size_t)E / 2];
    for (int c = 0; c < 4; c++) {
      obs[(size_t)E / 2] = keep;
      if (c == 0) obs[(size_t)E / 2].pose = P; else if (c == 1) obs[(size_t)E / 2].pose = -1; else if (c == 2) obs[(size_t)E / 2].point = L; else obs[(size_t)E / 2].point = -1;
      EXPECT(resident_lists_build(obs.data(), P, L, E, r) == 1);
    }
  }
  std::printf("P %d L %d E %d ok\n", P, L, E);
}

int main() {
  const int sizes[] = {0, 1, 63, 64, 65, 257};
  unsigned seed = 1;
  for (int L : sizes)
    for (int E : sizes) {
      if (L == 0 && E > 0) continue;                    // (no point to name)
      window(3, L, E, seed++);
    }
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("every list as the direct enumeration\n");
  return 0;
}
