// tools/check_kf_store_layout.cpp -- the slot layout of dvm_keyframe_store (dvm_slam_amd/csrc/kf_store_layout.h) over a set of
// slot_keypoints: every array of a slot starts at a multiple of 64 bytes, lies inside the slot stride, overlaps no other and holds the
// largest keyframe the slot admits (n = fv_n = features = slot_keypoints, 64 levels); the stride is a multiple of 64, so every slot of
// the block is aligned as the first; the staging bound covers every smaller keyframe.  Plain g++, no HIP header, nothing but the layout
// header (tests/test_keyframe_store_layout.py builds it, also with sanitizers).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../dvm_slam_amd/csrc/kf_store_layout.h"

using namespace dvm;

static int fails = 0;
static size_t g_K;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s  [slot_keypoints=%zu]\n", __FILE__, __LINE__, #c, g_K); fails++; } } while (0)

struct Item { const char* name; size_t at, bytes, need; };

int main() {
  const size_t sizes[] = {1, 63, 64, 65, 1024, 1900, 8192};
  for (size_t K : sizes) {
    g_K = K;
    const KfSlotLayout L = kf_slot_layout(K);
    const KfSlotBytes B = kf_slot_bytes(K);
    // need: the bytes of the largest keyframe, written out by hand (not taken from the header)
    std::vector<Item> items = {
        {"kps", L.kps, B.kps, K * 28},           {"desc", L.desc, B.desc, K * 32},
        {"fv_node", L.fv_node, B.fv_node, K * 4}, {"fv_off", L.fv_off, B.fv_off, (K + 1) * 4},
        {"fv_feat", L.fv_feat, B.fv_feat, K * 4}, {"sf", L.sf, B.sf, 64 * 4},
        {"sigma2", L.sigma2, B.sigma2, 64 * 4},   {"inv_sigma2", L.inv_sigma2, B.inv_sigma2, 64 * 4},
        {"skp", L.skp, B.skp, K * 16},            {"sidx", L.sidx, B.sidx, K * 4},
        {"sdesc", L.sdesc, B.sdesc, K * 32},      {"cell_start", L.cell_start, B.cell_start, (64 * 48 + 1) * 4},
        {"counters", L.counters, B.counters, 3 * 4}};
    EXPECT(items.size() == 13);
    for (const Item& it : items) {
      EXPECT(it.at % 64 == 0);
      EXPECT(it.bytes >= it.need);
      EXPECT(it.at + it.bytes <= L.stride);
    }
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.at < b.at; });
    for (size_t i = 1; i < items.size(); i++) EXPECT(items[i - 1].at + items[i - 1].bytes <= items[i].at);
    EXPECT(L.stride % 64 == 0 && L.stride > 0);
    // the staging bound: monotone in every count, so the largest keyframe bounds all
    EXPECT(kf_stage_bytes_max(K) == kf_stage_bytes(K, K, K, 64));
    const size_t ns[] = {0, 1, K / 2, K};
    for (size_t n : ns)
      for (size_t fv : {(size_t)0, n / 3, n})
        for (size_t nl : {(size_t)1, (size_t)8, (size_t)64}) {
          EXPECT(kf_stage_bytes(n, fv, n, nl) <= kf_stage_bytes_max(K));
          EXPECT(kf_stage_bytes(n, fv, n, nl) % 64 == 0);
        }
    std::printf("slot_keypoints %zu: stride %zu bytes\n", K, L.stride);
  }
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("every slot layout aligned, disjoint and large enough\n");
  return 0;
}
