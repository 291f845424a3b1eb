// tools/check_fuse_points_lists.cpp -- the host checks of the Fuse runs on map-store slots (dvm_slam_amd/csrc/fuse_points_lists.h) against a
// brute-force restatement: a call passes exactly when the direct enumeration finds no offence, a refused call names an offence the
// enumeration finds too, and after a pass every index the kernels form -- the record of a slot, the first-index table and the exclude
// marks at a slot, the flat index, the block of a flat index, a candidate's position -- lies inside its array (the kernels' walk is
// replayed on vectors of exactly the reserved sizes, every access through at()).  Calls at n of 0, 1, 63, 64, 65 and 257, for the
// resident run and for the candidates call with one and three lists, each offence planted in turn.  Plain g++, no HIP header
// (tests/test_fuse_points_lists.py builds it, also with sanitizers).
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../dvm_slam_amd/csrc/fuse_points_lists.h"

using namespace dvm;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Call {
  std::vector<std::vector<int32_t>> lists;       // the resident run: lists[0] is P.slot
  std::vector<int32_t> lens, exclude;
  std::vector<const int32_t*> ptrs;
  std::vector<uint8_t> written;
  bool with_store = true, null_list = false, null_lens = false, null_exclude = false;
  int n_lists_override = -2, n_exclude_override = -2, n_override = -2;
  int max_points = 0, max_entries = 0, table_capacity = 0;
  FplStore store() const { return FplStore{with_store ? (int32_t)written.size() : -1, with_store ? written.data() : nullptr}; }
  dvm_ft_points_resident points() const {
    dvm_ft_points_resident P{};
    P.n = n_override != -2 ? n_override : (int32_t)lists[0].size();
    P.slot = null_list ? nullptr : lists[0].data();
    return P;
  }
  dvm_ft_candidates cand() {
    ptrs.clear(); lens.clear();
    for (size_t l = 0; l < lists.size(); l++) { ptrs.push_back(null_list && l == 0 ? nullptr : lists[l].data()); lens.push_back((int32_t)lists[l].size()); }
    if (n_override != -2 && !lens.empty()) lens[0] = n_override;
    dvm_ft_candidates C{};
    C.n_lists = n_lists_override != -2 ? n_lists_override : (int32_t)lists.size();
    C.mp_slot = ptrs.data(); C.n = null_lens ? nullptr : lens.data();
    C.exclude = null_exclude ? nullptr : exclude.data();
    C.n_exclude = n_exclude_override != -2 ? n_exclude_override : (int32_t)exclude.size();
    return C;
  }
};

// every offence of a slot list, by direct enumeration
static void list_offences(const Call& c, const std::vector<int32_t>& a, std::set<int>& f) {
  for (int32_t sl : a) {
    if (sl == -1) continue;
    if (sl < -1) f.insert(kFplSlot);
    else if (!c.with_store) f.insert(kFplNoStore);
    else if (sl >= (int32_t)c.written.size() || !c.written[(size_t)sl]) f.insert(kFplSlot);
  }
}
static std::set<int> points_offences(const Call& c) {
  std::set<int> f;
  const int n = c.n_override != -2 ? c.n_override : (int)c.lists[0].size();
  if (n < 0) { f.insert(kFplCount); return f; }
  if (n > c.max_points) f.insert(kFplPoints);
  if (n > 0 && c.null_list) { f.insert(kFplNull); return f; }
  list_offences(c, c.lists[0], f);
  return f;
}
static std::set<int> cand_offences(const Call& c) {
  std::set<int> f;
  const int L = c.n_lists_override != -2 ? c.n_lists_override : (int)c.lists.size();
  const int X = c.n_exclude_override != -2 ? c.n_exclude_override : (int)c.exclude.size();
  if (L < 0 || X < 0) { f.insert(kFplCount); return f; }
  if ((L > 0 && c.null_lens) || (X > 0 && c.null_exclude)) { f.insert(kFplNull); return f; }
  int64_t total = 0;
  for (int l = 0; l < L; l++) {
    const int n = l == 0 && c.n_override != -2 ? c.n_override : (int)c.lists[(size_t)l].size();
    if (n < 0) { f.insert(kFplCount); return f; }
    if (n > 0 && c.null_list && l == 0) { f.insert(kFplNull); return f; }
    total += n;
  }
  if (total > c.max_points) f.insert(kFplPoints);
  if (total > c.max_entries || X > c.max_entries) f.insert(kFplEntries);
  if (c.with_store && (int)c.written.size() > c.table_capacity) f.insert(kFplTable);
  for (int l = 0; l < L; l++) list_offences(c, c.lists[(size_t)l], f);
  list_offences(c, c.exclude, f);
  return f;
}

// capacity 3 n + 7; every third slot never written; the lists name written slots in descending order with gaps, repeats inside and
// across lists, and -1 entries
static Call make(int n, int n_lists, unsigned seed) {
  std::mt19937 rng(seed);
  Call c;
  const int cap = 3 * n + 7;
  c.written.assign((size_t)cap, 1);
  for (int s = 2; s < cap; s += 3) c.written[(size_t)s] = 0;
  auto pick = [&]() { int s; do s = (int)(rng() % (unsigned)cap); while (!c.written[(size_t)s]); return s; };
  c.lists.resize((size_t)n_lists);
  for (int k = 0; k < n; k++) {
    const int32_t sl = k % 7 == 3 ? -1 : k % 5 == 4 && k > 4 ? c.lists[(size_t)((k - 5) % n_lists)][(size_t)((k - 5) / n_lists)] : (int32_t)pick();
    c.lists[(size_t)(k % n_lists)].push_back(sl);
  }
  for (int k = 0; k < (n + 1) / 2; k++) c.exclude.push_back(k % 4 == 1 ? -1 : (int32_t)pick());
  for (auto& a : c.lists) a.reserve(a.size() + 1);
  c.exclude.reserve(c.exclude.size() + 1);
  c.max_points = n + 3; c.max_entries = n + 2; c.table_capacity = cap;
  return c;
}

template <class V, class O> static void expect_refused(const V& v, const O& f, int fault, int rc, const char* what) {
  if (!(v.fault != kFplOk && f.count(v.fault) && f.count(fault) && v.rc() != DVM_OK && (v.fault != fault || v.rc() == rc))) {
    std::printf("FAILED: %s: verdict %d rc %d\n", what, v.fault, v.rc());
    fails++;
  }
}
static void refused_points(const Call& c, int fault, int rc, const char* what) { expect_refused(fpl_check_points(c.points(), c.store(), c.max_points), points_offences(c), fault, rc, what); }
static void refused_cand(Call c, int fault, int rc, const char* what) {
  const FplVerdict v = fpl_check_candidates(c.cand(), c.store(), c.max_points, c.max_entries, c.table_capacity);
  expect_refused(v, cand_offences(c), fault, rc, what);
}

// the walk of k_ft_gather over a passed resident call
static void replay_gather(const Call& c, const std::vector<int32_t>& slot, int n) {
  std::vector<uint32_t> records(c.with_store ? c.written.size() * 18 : 0), pos((size_t)c.max_points * 3), desc((size_t)c.max_points * 8);
  std::vector<uint8_t> valid((size_t)c.max_points);
  for (int k = 0; k < n; k++) {
    const int32_t sl = slot.at((size_t)k);
    if (sl < 0) { valid.at((size_t)k) = 0; continue; }
    for (int w = 0; w < 18; w++) (void)records.at((size_t)sl * 18 + (size_t)w);
    pos.at(3 * (size_t)k + 2) = 0; desc.at(8 * (size_t)k + 7) = 0; valid.at((size_t)k) = 1;
  }
}
// the walk of k_ft_cand_mark / count / write / reset and of the gather behind them over a passed candidates call; the list it makes
// against the definition (not bad is every record here: the bad flag is read on the device)
static void replay_candidates(Call& c) {
  const dvm_ft_candidates C = c.cand();
  const FplVerdict v = fpl_check_candidates(C, c.store(), c.max_points, c.max_entries, c.table_capacity);
  EXPECT(v.fault == kFplOk);
  const int M = (int)v.total;
  std::vector<int32_t> entry((size_t)M), first((size_t)c.table_capacity, 0x7f7f7f7f), cand((size_t)c.max_entries);
  std::vector<uint8_t> mark((size_t)c.table_capacity, 0);
  std::vector<uint32_t> records(c.with_store ? c.written.size() * 18 : 0);
  if (M) fpl_flatten(C, entry.data());
  { size_t at = 0; for (auto& a : c.lists) for (int32_t sl : a) EXPECT(entry.at(at++) == sl); EXPECT(at == (size_t)M); }
  for (int i = 0; i < M; i++) {
    const int32_t sl = entry.at((size_t)i);
    if (sl >= 0) { (void)records.at((size_t)sl * 18 + 17); if (first.at((size_t)sl) > i) first.at((size_t)sl) = i; }
  }
  for (int32_t sl : c.exclude) if (sl >= 0) mark.at((size_t)sl) = 1;
  const size_t blocks = ((size_t)M + 255) / 256, max_blocks = ((size_t)c.max_entries + 255) / 256;
  std::vector<int32_t> cnt(max_blocks, 0), off(max_blocks + 1, 0);
  for (int i = 0; i < M; i++) { const int32_t sl = entry.at((size_t)i); if (sl >= 0 && first.at((size_t)sl) == i) cnt.at((size_t)i / 256)++; }
  for (size_t b = 0; b < blocks; b++) off.at(b + 1) = off.at(b) + cnt.at(b);
  std::vector<int32_t> at(off);
  for (int i = 0; i < M; i++) { const int32_t sl = entry.at((size_t)i); if (sl >= 0 && first.at((size_t)sl) == i) cand.at((size_t)at.at((size_t)i / 256)++) = sl; }
  const int n_cand = off.at(blocks);
  std::vector<int32_t> want;                        // the definition: first occurrence, flat order
  for (int i = 0; i < M; i++) {
    bool seen = entry[(size_t)i] < 0;
    for (int j = 0; j < i && !seen; j++) seen = entry[(size_t)j] == entry[(size_t)i];
    if (!seen) want.push_back(entry[(size_t)i]);
  }
  EXPECT(n_cand == (int)want.size() && n_cand <= M);
  for (int k = 0; k < n_cand && k < (int)want.size(); k++) EXPECT(cand.at((size_t)k) == want[(size_t)k]);
  std::vector<uint8_t> valid((size_t)c.max_points);
  for (int k = 0; k < M; k++) {                     // the gather over the bound: rows beyond the count read no slot
    if (k >= n_cand) { valid.at((size_t)k) = 0; continue; }
    const int32_t sl = cand.at((size_t)k);
    (void)records.at((size_t)sl * 18 + 17);
    valid.at((size_t)k) = mark.at((size_t)sl) ? 0 : 1;
  }
  for (int i = 0; i < M; i++) { const int32_t sl = entry.at((size_t)i); if (sl >= 0) first.at((size_t)sl) = 0x7f7f7f7f; }
  for (int32_t sl : c.exclude) if (sl >= 0) mark.at((size_t)sl) = 0;
  for (int32_t x : first) EXPECT(x == 0x7f7f7f7f);   // both tables idle again
  for (uint8_t x : mark) EXPECT(x == 0);
}

static void call(int n, unsigned seed) {
  // ---- the resident run
  Call c = make(n, 1, seed);
  EXPECT(points_offences(c).empty());
  { const FplVerdict v = fpl_check_points(c.points(), c.store(), c.max_points); EXPECT(v.fault == kFplOk && v.rc() == DVM_OK); }
  replay_gather(c, c.lists[0], n);
  { Call d = c; for (auto& sl : d.lists[0]) sl = -1; d.with_store = false;      // no store, no point named: legal
    EXPECT(points_offences(d).empty() && fpl_check_points(d.points(), d.store(), d.max_points).fault == kFplOk); replay_gather(d, d.lists[0], n); }
  { Call d = c; d.n_override = -1; refused_points(d, kFplCount, DVM_ERR_INVALID, "n -1"); }
  { Call d = c; d.max_points = n - 1; if (n) refused_points(d, kFplPoints, DVM_ERR_CAPACITY, "n beyond max_points"); }
  if (n) { Call d = c; d.null_list = true; refused_points(d, kFplNull, DVM_ERR_INVALID, "slot NULL"); }
  for (int k = 0; k < n; k += (k >= 8 && k < n - 3 ? n / 7 : 1)) {
    const int cap = (int)c.written.size();
    { Call d = c; d.lists[0][(size_t)k] = cap; refused_points(d, kFplSlot, DVM_ERR_INVALID, "slot = capacity"); d.lists[0][(size_t)k] = -2; refused_points(d, kFplSlot, DVM_ERR_INVALID, "slot -2"); }
    { Call d = c; d.lists[0][(size_t)k] = 2; refused_points(d, kFplSlot, DVM_ERR_INVALID, "slot never written"); }
    { Call d = c; d.lists[0][(size_t)k] = 0; d.with_store = false; refused_points(d, kFplNoStore, DVM_ERR_INVALID, "slot without a store"); }
  }
  // ---- the candidates call, one list and three
  for (int n_lists : {1, 3}) {
    Call e = make(n, n_lists, seed + 100);
    EXPECT(cand_offences(e).empty());
    replay_candidates(e);
    { Call d = e; d.n_lists_override = -1; refused_cand(d, kFplCount, DVM_ERR_INVALID, "n_lists -1"); }
    { Call d = e; d.n_exclude_override = -1; refused_cand(d, kFplCount, DVM_ERR_INVALID, "n_exclude -1"); }
    { Call d = e; d.n_override = -1; refused_cand(d, kFplCount, DVM_ERR_INVALID, "a list's n -1"); }
    { Call d = e; d.null_lens = true; refused_cand(d, kFplNull, DVM_ERR_INVALID, "n NULL"); }
    if (!e.lists[0].empty()) { Call d = e; d.null_list = true; refused_cand(d, kFplNull, DVM_ERR_INVALID, "a list NULL"); }
    if (!e.exclude.empty()) { Call d = e; d.null_exclude = true; refused_cand(d, kFplNull, DVM_ERR_INVALID, "exclude NULL"); }
    if (n) { Call d = e; d.max_points = n - 1; refused_cand(d, kFplPoints, DVM_ERR_CAPACITY, "total beyond max_points"); }
    if (n) { Call d = e; d.max_entries = n - 1; refused_cand(d, kFplEntries, DVM_ERR_CAPACITY, "total beyond max_entries"); }
    if (!e.exclude.empty()) { Call d = e; d.max_entries = (int)d.exclude.size() - 1; refused_cand(d, kFplEntries, DVM_ERR_CAPACITY, "n_exclude beyond max_entries"); }
    { Call d = e; d.table_capacity = (int)d.written.size() - 1; refused_cand(d, kFplTable, DVM_ERR_CAPACITY, "store beyond map_capacity"); }
    const int cap = (int)e.written.size();
    for (size_t l = 0; l <= e.lists.size(); l++) {
      std::vector<int32_t>& a0 = l < e.lists.size() ? e.lists[l] : e.exclude;
      for (size_t k = 0; k < a0.size(); k += (k >= 8 && k + 3 < a0.size() ? a0.size() / 7 : 1)) {
        Call d = e;
        std::vector<int32_t>& a = l < d.lists.size() ? d.lists[l] : d.exclude;
        a[k] = cap; refused_cand(d, kFplSlot, DVM_ERR_INVALID, "slot = capacity");
        a[k] = -2; refused_cand(d, kFplSlot, DVM_ERR_INVALID, "slot -2");
        a[k] = 2; refused_cand(d, kFplSlot, DVM_ERR_INVALID, "slot never written");
        a[k] = 0; d.with_store = false; refused_cand(d, kFplNoStore, DVM_ERR_INVALID, "slot without a store");
      }
    }
  }
  std::printf("n %d ok\n", n);
}

int main() {
  const int sizes[] = {0, 1, 63, 64, 65, 257};
  unsigned seed = 1;
  for (int n : sizes) call(n, seed++);
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("every verdict as the direct enumeration\n");
  return 0;
}
