// tools/check_fv_once.cpp -- dvm_slam_amd/csrc/fv_once.h as a plain program: fv_first_repeat against a quadratic restatement over
// FeatureVectors of n keypoints that list every feature once, leave some out, or list one a second time (first, last, adjacent or
// far apart), with the scratch array exactly n bytes on the heap so that a sanitizer build sees any step outside it.
// Build: g++ -std=c++17 -O2 -Wall -Werror tools/check_fv_once.cpp (tests/test_bow_store_abi.py also builds it with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "../dvm_slam_amd/csrc/fv_once.h"

namespace {
int32_t slow_first_repeat(const std::vector<int32_t>& f) {
  for (size_t p = 0; p < f.size(); p++)
    for (size_t q = 0; q < p; q++)
      if (f[q] == f[p]) return f[p];
  return -1;
}
}  // namespace

int main() {
  std::mt19937 rng(12345);
  int cases = 0, repeats = 0;
  for (int n : {0, 1, 2, 3, 63, 64, 65, 257, 1149, 8192}) {
    for (int round = 0; round < (n > 2000 ? 6 : 40); round++) {
      std::vector<int32_t> perm((size_t)n);
      for (int i = 0; i < n; i++) perm[(size_t)i] = i;
      for (int i = n - 1; i > 0; i--) std::swap(perm[(size_t)i], perm[rng() % (uint32_t)(i + 1)]);
      const int listed = n == 0 ? 0 : (round % 4 == 0 ? n : (int)(rng() % (uint32_t)(n + 1)));   // a put admits at most n listed features
      std::vector<int32_t> f(perm.begin(), perm.begin() + listed);
      if (listed >= 2 && round % 3 != 0) {                                                      // one feature a second time
        const size_t to = round % 3 == 1 ? (size_t)listed - 1 : rng() % (size_t)listed;
        size_t from = round % 6 == 1 ? 0 : rng() % (size_t)listed;
        if (from == to) from = (to + 1) % (size_t)listed;
        f[to] = f[from];
      }
      std::unique_ptr<uint8_t[]> seen(new uint8_t[(size_t)n ? (size_t)n : 1]);
      for (int i = 0; i < n; i++) seen[(size_t)i] = 0xAB;                                       // (the scan clears what it uses)
      const int32_t got = dvm::fv_first_repeat(f.data(), (int32_t)f.size(), n, seen.get());
      const int32_t want = slow_first_repeat(f);
      if (got != want) {
        std::printf("n = %d round %d: fv_first_repeat %d, restated %d\n", n, round, got, want);
        return 1;
      }
      cases++; repeats += want >= 0;
    }
  }
  if (repeats == 0 || repeats == cases) { std::printf("the cases do not cover both answers\n"); return 1; }
  std::printf("fv_first_repeat agrees on %d feature vectors (%d with a repeat)\n", cases, repeats);
  return 0;
}
