// tools/check_update_local_map_lists.cpp -- the host checks of dvm_update_local_map (dvm_slam_amd/csrc/update_local_map_lists.h) against a
// brute-force restatement: a call passes exactly when the direct enumeration finds no offence, a refused call names an offence the
// enumeration finds too, and after a pass every index the k_ulm_* kernels form lies inside its array -- the kernels' walk is replayed on
// vectors of exactly the reserved sizes, every access through at(): mult, the votes, the keys, the workgroup counts and offsets, the
// list, pos, frame_mp, the resets, and all three tables idle at the end.  The replayed results are held against the definitions (votes[j]
// = the sum of mult over the OBSERVED row; the MATCHES entries that are live and the first of their slot, in flat order).  Frames of 0,
// 1, 63, 64, 65, 257 and 1 025 keypoints with 0, 1, 3 and 9 named keyframes, each offence planted in turn, in the LAST frame slot of a
// reservation of three.  Plain g++, no HIP header (tests/test_update_local_map_lists.py builds it, also with sanitizers).
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../dvm_slam_amd/csrc/update_local_map_lists.h"

using namespace dvm;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Scene {
  UlmReserve R{};
  int map_cap = 0, kf_cap = 0, K = 0;
  std::vector<uint8_t> written, bad;               // [map_cap]
  std::vector<int32_t> len;                        // [kf_cap] MATCHES == OBSERVED lengths (0: no row)
  std::vector<uint8_t> kf_there, has_row, other_store;   // [kf_cap]
  std::vector<int32_t> matches, observed;          // [kf_cap][row_words]
  size_t row_words = 0;
  std::vector<int32_t> mp_slot, kf_slot;
  std::vector<int32_t> votes_out, local_out, frame_mp_out;
  std::vector<uint8_t> bad_out;
  bool same_device = true, observed_same = true, null_mp = false, null_kf = false, null_out = false;
  int n_override = -2, n_kfs_override = -2, local_cap = 0;
  std::vector<uint8_t> state;
  UlmFacts facts() {
    state.assign(kf_slot.size(), kUlmKfGood);
    for (size_t k = 0; k < kf_slot.size(); k++) {
      const int32_t sl = kf_slot[k];
      state[k] = sl < 0 || sl >= kf_cap || !kf_there[(size_t)sl] ? kUlmKfAbsent : !has_row[(size_t)sl] ? kUlmKfRowless : other_store[(size_t)sl] ? kUlmKfOtherStore : kUlmKfGood;
    }
    return UlmFacts{same_device, map_cap, written.data(), kf_cap, K, observed_same, state.data()};
  }
  int n() const { return n_override != -2 ? n_override : (int)mp_slot.size(); }
  int n_kfs() const { return n_kfs_override != -2 ? n_kfs_override : (int)kf_slot.size(); }
  dvm_ulm_keyframes_in kin() const { return dvm_ulm_keyframes_in{(const dvm_keyframe_store*)this, (const dvm_map_store*)this, n(), null_mp ? nullptr : mp_slot.data()}; }
  dvm_ulm_keyframes_out kout() { return dvm_ulm_keyframes_out{null_out ? nullptr : votes_out.data(), bad_out.data()}; }
  dvm_ulm_points_in pin() const {
    return dvm_ulm_points_in{(const dvm_keyframe_store*)this, (const dvm_map_store*)this, n_kfs(), null_kf ? nullptr : kf_slot.data(), n(), null_mp ? nullptr : mp_slot.data()};
  }
  dvm_ulm_points_out pout() { return dvm_ulm_points_out{local_out.data(), local_cap, 0, null_out ? nullptr : frame_mp_out.data(), 0}; }
};

static Scene make(int n, int n_kfs, unsigned seed) {
  std::mt19937 rng(seed);
  Scene s;
  s.map_cap = 3 * n + 40; s.kf_cap = n_kfs + 6; s.K = 300;
  s.R = UlmReserve{3, n + 2, n_kfs + 1, s.map_cap + 3, s.kf_cap + 1, s.K + 20};
  s.row_words = ulm_pad16((size_t)s.K);
  s.written.assign((size_t)s.map_cap, 1); s.bad.assign((size_t)s.map_cap, 0);
  for (int i = 2; i < s.map_cap; i += 3) s.written[(size_t)i] = 0;
  for (int i = 0; i < s.map_cap; i += 5) s.bad[(size_t)i] = 1;
  auto pick = [&]() { int v; do v = (int)(rng() % (unsigned)s.map_cap); while (!s.written[(size_t)v]); return (int32_t)v; };
  s.len.assign((size_t)s.kf_cap, 0); s.kf_there.assign((size_t)s.kf_cap, 1); s.has_row.assign((size_t)s.kf_cap, 1); s.other_store.assign((size_t)s.kf_cap, 0);
  s.kf_there[(size_t)s.kf_cap - 1] = 0; s.has_row[(size_t)s.kf_cap - 2] = 0; s.other_store[(size_t)s.kf_cap - 3] = 1;
  s.matches.assign((size_t)s.kf_cap * s.row_words, -1); s.observed = s.matches;
  const int lens[] = {300, 0, 1, 255, 256, 257, 64, 17, 299};
  for (int j = 0; j < s.kf_cap; j++) {
    if (!s.kf_there[(size_t)j] || !s.has_row[(size_t)j]) continue;
    s.len[(size_t)j] = lens[(size_t)j % 9];
    for (int kp = 0; kp < s.len[(size_t)j]; kp++) {
      if (rng() % 4) s.matches[(size_t)j * s.row_words + (size_t)kp] = pick();
      if (rng() % 3) s.observed[(size_t)j * s.row_words + (size_t)kp] = pick();
    }
  }
  for (int i = 0; i < n; i++) s.mp_slot.push_back(i % 6 == 2 ? -1 : i % 9 == 8 && i > 8 ? s.mp_slot[(size_t)i - 9] : pick());
  for (int k = 0; k < n_kfs; k++) s.kf_slot.push_back((int32_t)((k * 5 + 1) % (s.kf_cap - 3)));   // distinct for n_kfs <= kf_cap - 3, never the three odd ones
  s.mp_slot.reserve((size_t)n + 1); s.kf_slot.reserve((size_t)n_kfs + 1);
  s.votes_out.assign((size_t)s.kf_cap, 0); s.bad_out.assign((size_t)n + 1, 0); s.frame_mp_out.assign((size_t)n + 1, 0);
  s.local_cap = s.map_cap; s.local_out.assign((size_t)s.map_cap, 0);
  return s;
}

// every offence of a call, by direct enumeration
static void common_offences(Scene& s, std::set<int>& f) {
  if (!s.same_device) f.insert(kUlmDevice);
  if (s.n() > s.R.max_frame_keypoints) f.insert(kUlmKeypoints);
  if (s.map_cap > s.R.map_capacity) f.insert(kUlmMapTable);
  if (s.kf_cap > s.R.kf_capacity) f.insert(kUlmKfTable);
  if (s.K > s.R.slot_keypoints) f.insert(kUlmSlotKeypoints);
  for (int32_t sl : s.mp_slot)
    if (sl != -1 && (sl < -1 || sl >= s.map_cap || !s.written[(size_t)sl])) f.insert(kUlmFrameSlot);
}
static std::set<int> keyframes_offences(Scene& s) {
  std::set<int> f;
  if (s.null_out || (s.n() > 0 && s.null_mp)) { f.insert(kUlmNull); return f; }
  if (s.n() < 0) { f.insert(kUlmCount); return f; }
  common_offences(s, f);
  if (!s.observed_same) f.insert(kUlmObservedStore);
  return f;
}
static std::set<int> points_offences(Scene& s) {
  std::set<int> f;
  if ((s.n() > 0 && (s.null_out || s.null_mp)) || (s.n_kfs() > 0 && s.null_kf)) { f.insert(kUlmNull); return f; }
  if (s.n() < 0 || s.n_kfs() < 0 || s.local_cap < 0) { f.insert(kUlmCount); return f; }
  if (s.n_kfs() > s.R.max_local_keyframes) f.insert(kUlmLocalKfs);
  common_offences(s, f);
  std::set<int32_t> seen;
  for (int32_t sl : s.kf_slot) {
    if (sl < 0 || sl >= s.kf_cap || !s.kf_there[(size_t)sl]) { f.insert(kUlmKfSlot); continue; }
    if (!s.has_row[(size_t)sl]) f.insert(kUlmKfNoRow);
    if (s.other_store[(size_t)sl]) f.insert(kUlmRowStore);
    if (!seen.insert(sl).second) f.insert(kUlmKfTwice);
  }
  return f;
}
static void refused(const UlmVerdict& v, const std::set<int>& f, int fault, int rc, const char* what) {
  if (!(v.fault != kUlmOk && f.count(v.fault) && f.count(fault) && v.rc() != DVM_OK && (v.fault != fault || v.rc() == rc) && v.frame == 2)) {
    std::printf("FAILED: %s: verdict %d rc %d frame %d\n", what, v.fault, v.rc(), v.frame);
    fails++;
  }
}
static std::vector<uint32_t> g_stamp;
static uint32_t g_call = 0;
static UlmVerdict check_points(Scene& s) {
  g_stamp.resize((size_t)s.R.kf_capacity, 0u);
  const UlmFacts F = s.facts();
  return ulm_check_points_frame(s.R, F, 2, s.pin(), s.pout(), g_stamp.data(), ++g_call);
}
static UlmVerdict check_keyframes(Scene& s) { const UlmFacts F = s.facts(); return ulm_check_keyframes_frame(s.R, F, 2, s.kin(), s.kout()); }
static void refused_k(Scene s, int fault, int rc, const char* what) { refused(check_keyframes(s), keyframes_offences(s), fault, rc, what); }
static void refused_p(Scene s, int fault, int rc, const char* what) { refused(check_points(s), points_offences(s), fault, rc, what); }

// ---- the kernels' walk on vectors of the reserved sizes, frame b = 2 of 3
struct Tables {
  std::vector<int32_t> mult, first, pos, cnt, off, lists, votes, local, frame_mp;
  std::vector<uint8_t> frame_bad;
  size_t M, blocks_max, n_pad;
  int RB;
  explicit Tables(const UlmReserve& R) {
    M = (size_t)R.map_capacity; RB = ulm_row_blocks(R.slot_keypoints); blocks_max = (size_t)R.max_local_keyframes * (size_t)RB;
    n_pad = ulm_pad16((size_t)R.max_frame_keypoints);
    const size_t F = (size_t)R.max_frames;
    mult.assign(F * M, 0); first.assign(F * M, kUlmFirstIdle); pos.assign(F * M, -1);
    cnt.assign(F * (blocks_max + 1), 0); off.assign(F * (blocks_max + 1), 0);
    lists.assign(F * (ulm_pad16((size_t)R.max_frame_keypoints) + ulm_pad16((size_t)R.max_local_keyframes)), 0);
    votes.assign(F * (size_t)R.kf_capacity, -7); local.assign(F * M, -7); frame_mp.assign(F * n_pad, -7); frame_bad.assign(F * n_pad, 7);
  }
  void idle() const {
    for (int32_t x : mult) EXPECT(x == 0);
    for (int32_t x : first) EXPECT(x == kUlmFirstIdle);
    for (int32_t x : pos) EXPECT(x == -1);
  }
};

static void replay_keyframes(Scene& s, Tables& T) {
  const size_t b = 2, n = (size_t)s.n();
  // the upload: three parameter blocks, then the lists; frames 0 and 1 carry the largest lists the reservation allows
  dvm_ulm_keyframes_in in[3] = {s.kin(), s.kin(), s.kin()};
  in[0].n = in[1].n = s.R.max_frame_keypoints;
  const size_t mp_off = 2 * ulm_pad16((size_t)s.R.max_frame_keypoints);
  EXPECT(ulm_keyframes_upload_bytes(3, in) == 3 * kUlmParamBytes + 4 * (mp_off + ulm_pad16(n)));
  EXPECT(mp_off + ulm_pad16(n) <= T.lists.size());
  for (size_t i = 0; i < n; i++) T.lists.at(mp_off + i) = s.mp_slot.at(i);
  std::vector<uint32_t> records((size_t)s.map_cap * 18, 0);
  for (int i = 0; i < s.map_cap; i++) records.at((size_t)i * 18 + 17) = s.bad[(size_t)i];
  for (size_t i = 0; i < n; i++) {                                   // k_ulm_mult
    const int32_t sl = T.lists.at(mp_off + i);
    const bool bad = sl >= 0 && records.at((size_t)sl * 18 + 17) != 0;
    T.frame_bad.at(b * T.n_pad + i) = bad;
    if (sl >= 0 && !bad) T.mult.at(b * T.M + (size_t)sl)++;
  }
  for (int j = 0; j < s.kf_cap; j++) {                               // k_ulm_votes: 16-byte loads, 64 lanes
    const int len = s.len.at((size_t)j);
    int sum = 0;
    for (int lane = 0; lane < 64; lane++)
      for (int i = lane * 4; i < len; i += 256)
        for (int c = 0; c < 4; c++) {
          const int32_t v = s.observed.at((size_t)j * s.row_words + (size_t)(i + c));   // (the whole load lies inside the row's words)
          if (i + c < len && v >= 0) sum += T.mult.at(b * T.M + (size_t)v);
        }
    T.votes.at(b * (size_t)s.R.kf_capacity + (size_t)j) = sum;
  }
  for (size_t i = 0; i < n; i++) { const int32_t sl = T.lists.at(mp_off + i); if (sl >= 0) T.mult.at(b * T.M + (size_t)sl) = 0; }   // k_ulm_mult_reset
  // the definition
  for (int j = 0; j < s.kf_cap; j++) {
    int want = 0;
    for (int kp = 0; kp < s.len[(size_t)j]; kp++) {
      const int32_t v = s.observed[(size_t)j * s.row_words + (size_t)kp];
      if (v < 0 || s.bad[(size_t)v]) continue;
      for (int32_t sl : s.mp_slot) want += sl == v;
    }
    EXPECT(T.votes.at(b * (size_t)s.R.kf_capacity + (size_t)j) == want);
  }
  for (size_t i = 0; i < n; i++) EXPECT(T.frame_bad.at(b * T.n_pad + i) == (s.mp_slot[i] >= 0 && s.bad[(size_t)s.mp_slot[i]]));
  T.idle();
}

static void replay_points(Scene& s, Tables& T, int local_cap) {
  const size_t b = 2, n = (size_t)s.n(), nk = (size_t)s.n_kfs();
  T.local.assign(T.local.size(), -7);                               // (the caller's array: fresh per call)
  dvm_ulm_points_in in[3] = {s.pin(), s.pin(), s.pin()};
  in[0].n = in[1].n = s.R.max_frame_keypoints; in[0].n_kfs = in[1].n_kfs = s.R.max_local_keyframes;
  const size_t mp_off = 2 * (ulm_pad16((size_t)s.R.max_frame_keypoints) + ulm_pad16((size_t)s.R.max_local_keyframes)), kf_off = mp_off + ulm_pad16(n);
  EXPECT(ulm_points_upload_bytes(3, in) == 3 * kUlmParamBytes + 4 * (kf_off + ulm_pad16(nk)));
  EXPECT(kf_off + ulm_pad16(nk) <= T.lists.size());
  for (size_t i = 0; i < n; i++) T.lists.at(mp_off + i) = s.mp_slot.at(i);
  for (size_t k = 0; k < nk; k++) T.lists.at(kf_off + k) = s.kf_slot.at(k);
  const int RB = T.RB, blocks = (int)nk * RB;
  auto entry = [&](int x, int tid) -> int32_t {                      // ulm_entry
    const int k = x / RB;
    if (k >= (int)nk) return -1;
    const int kp = (x - k * RB) * kUlmBlock + tid;
    const int32_t j = T.lists.at(kf_off + (size_t)k);
    return kp < s.len.at((size_t)j) ? s.matches.at((size_t)j * s.row_words + (size_t)kp) : -1;
  };
  for (int x = 0; x < blocks; x++)                                   // k_ulm_mark
    for (int tid = 0; tid < kUlmBlock; tid++) {
      const int32_t sl = entry(x, tid);
      const int32_t key = x * kUlmBlock + tid;
      EXPECT(key < kUlmFirstIdle);
      if (sl >= 0 && !s.bad.at((size_t)sl) && T.first.at(b * T.M + (size_t)sl) > key) T.first.at(b * T.M + (size_t)sl) = key;
    }
  auto taken = [&](int x, int tid, int32_t sl) { return sl >= 0 && T.first.at(b * T.M + (size_t)sl) == x * kUlmBlock + tid; };
  for (int x = 0; x < blocks; x++) {                                 // k_ulm_count
    int c = 0;
    for (int tid = 0; tid < kUlmBlock; tid++) c += taken(x, tid, entry(x, tid));
    T.cnt.at(b * (T.blocks_max + 1) + (size_t)x) = c;
  }
  int base = 0;                                                      // k_ulm_scan
  for (int x = 0; x < blocks; x++) { T.off.at(b * (T.blocks_max + 1) + (size_t)x) = base; base += T.cnt.at(b * (T.blocks_max + 1) + (size_t)x); }
  T.off.at(b * (T.blocks_max + 1) + (size_t)blocks) = base;
  const int n_local = base;
  for (int x = 0; x < blocks; x++) {                                 // k_ulm_write
    int p = T.off.at(b * (T.blocks_max + 1) + (size_t)x);
    for (int tid = 0; tid < kUlmBlock; tid++) {
      const int32_t sl = entry(x, tid);
      if (!taken(x, tid, sl)) continue;
      T.pos.at(b * T.M + (size_t)sl) = p;
      if (p < local_cap) T.local.at(b * T.M + (size_t)p) = sl;
      p++;
    }
  }
  int outside = 0;                                                   // k_ulm_frame_mp
  for (size_t i = 0; i < n; i++) {
    const int32_t sl = T.lists.at(mp_off + i);
    int32_t p = -1;
    if (sl >= 0 && !s.bad.at((size_t)sl)) { p = T.pos.at(b * T.M + (size_t)sl); outside += p < 0; }
    T.frame_mp.at(b * T.n_pad + i) = p;
  }
  // the definition: the live entries in flat order, each slot once
  std::vector<int32_t> want;
  for (size_t k = 0; k < nk; k++) {
    const int32_t j = s.kf_slot[k];
    for (int kp = 0; kp < s.len[(size_t)j]; kp++) {
      const int32_t v = s.matches[(size_t)j * s.row_words + (size_t)kp];
      if (v < 0 || s.bad[(size_t)v]) continue;
      bool seen = false;
      for (int32_t w : want) seen |= w == v;
      if (!seen) want.push_back(v);
    }
  }
  EXPECT(n_local == (int)want.size() && n_local <= s.map_cap);
  for (int k = 0; k < n_local && k < (int)want.size(); k++) {
    if (k < local_cap) EXPECT(T.local.at(b * T.M + (size_t)k) == want[(size_t)k]);
    else EXPECT(T.local.at(b * T.M + (size_t)k) == -7);              // nothing past local_cap
  }
  int want_outside = 0;
  for (size_t i = 0; i < n; i++) {
    const int32_t sl = s.mp_slot[i];
    int32_t p = -1;
    if (sl >= 0 && !s.bad[(size_t)sl]) {
      for (size_t k = 0; k < want.size(); k++) if (want[k] == sl) p = (int32_t)k;
      want_outside += p < 0;
    }
    EXPECT(T.frame_mp.at(b * T.n_pad + i) == p);
  }
  EXPECT(outside == want_outside);
  for (int x = 0; x < blocks; x++)                                   // k_ulm_points_reset
    for (int tid = 0; tid < kUlmBlock; tid++) {
      const int32_t sl = entry(x, tid);
      if (sl < 0) continue;
      T.first.at(b * T.M + (size_t)sl) = kUlmFirstIdle; T.pos.at(b * T.M + (size_t)sl) = -1;
    }
  T.idle();
}

static void call(int n, int n_kfs, unsigned seed) {
  Scene s = make(n, n_kfs, seed);
  EXPECT(ulm_check_reserve(s.R).fault == kUlmOk);
  EXPECT(keyframes_offences(s).empty() && points_offences(s).empty());
  EXPECT(check_keyframes(s).fault == kUlmOk && check_points(s).fault == kUlmOk);
  { Tables T(s.R); replay_keyframes(s, T); replay_points(s, T, s.map_cap); replay_points(s, T, 1); replay_keyframes(s, T); }
  // ---- each offence in turn, both calls
  { Scene d = s; d.n_override = -1; refused_k(d, kUlmCount, DVM_ERR_INVALID, "n -1"); refused_p(d, kUlmCount, DVM_ERR_INVALID, "n -1"); }
  if (n) { Scene d = s; d.null_mp = true; refused_k(d, kUlmNull, DVM_ERR_INVALID, "mp_slot NULL"); refused_p(d, kUlmNull, DVM_ERR_INVALID, "mp_slot NULL"); }
  { Scene d = s; d.null_out = true; refused_k(d, kUlmNull, DVM_ERR_INVALID, "votes NULL"); if (n) refused_p(d, kUlmNull, DVM_ERR_INVALID, "frame_mp NULL"); }
  { Scene d = s; d.same_device = false; refused_k(d, kUlmDevice, DVM_ERR_INVALID, "device"); refused_p(d, kUlmDevice, DVM_ERR_INVALID, "device"); }
  if (n) { Scene d = s; d.R.max_frame_keypoints = n - 1; refused_k(d, kUlmKeypoints, DVM_ERR_CAPACITY, "n"); refused_p(d, kUlmKeypoints, DVM_ERR_CAPACITY, "n"); }
  { Scene d = s; d.R.map_capacity = s.map_cap - 1; refused_k(d, kUlmMapTable, DVM_ERR_CAPACITY, "map"); refused_p(d, kUlmMapTable, DVM_ERR_CAPACITY, "map"); }
  { Scene d = s; d.R.kf_capacity = s.kf_cap - 1; refused_k(d, kUlmKfTable, DVM_ERR_CAPACITY, "kf"); }
  { Scene d = s; d.R.slot_keypoints = s.K - 1; refused_k(d, kUlmSlotKeypoints, DVM_ERR_CAPACITY, "K"); refused_p(d, kUlmSlotKeypoints, DVM_ERR_CAPACITY, "K"); }
  { Scene d = s; d.observed_same = false; refused_k(d, kUlmObservedStore, DVM_ERR_INVALID, "observed"); }
  for (int k = 0; k < n; k += (k >= 8 && k < n - 3 ? n / 7 : 1))
    for (int32_t v : {s.map_cap, -2, 2}) {
      Scene d = s; d.mp_slot[(size_t)k] = v;
      refused_k(d, kUlmFrameSlot, DVM_ERR_INVALID, "frame slot"); refused_p(d, kUlmFrameSlot, DVM_ERR_INVALID, "frame slot");
    }
  { Scene d = s; d.n_kfs_override = -1; refused_p(d, kUlmCount, DVM_ERR_INVALID, "n_kfs -1"); }
  { Scene d = s; d.local_cap = -1; refused_p(d, kUlmCount, DVM_ERR_INVALID, "local_cap -1"); }
  if (n_kfs) { Scene d = s; d.null_kf = true; refused_p(d, kUlmNull, DVM_ERR_INVALID, "kf_slot NULL"); }
  if (n_kfs) { Scene d = s; d.R.max_local_keyframes = n_kfs - 1; refused_p(d, kUlmLocalKfs, DVM_ERR_CAPACITY, "n_kfs"); }
  for (int k = 0; k < n_kfs; k++) {
    { Scene d = s; d.kf_slot[(size_t)k] = s.kf_cap; refused_p(d, kUlmKfSlot, DVM_ERR_INVALID, "kf_slot = capacity"); }
    { Scene d = s; d.kf_slot[(size_t)k] = -1; refused_p(d, kUlmKfSlot, DVM_ERR_INVALID, "kf_slot -1"); }
    { Scene d = s; d.kf_slot[(size_t)k] = s.kf_cap - 1; refused_p(d, kUlmKfSlot, DVM_ERR_INVALID, "kf_slot never put"); }
    { Scene d = s; d.kf_slot[(size_t)k] = s.kf_cap - 2; refused_p(d, kUlmKfNoRow, DVM_ERR_INVALID, "kf_slot without a row"); }
    { Scene d = s; d.kf_slot[(size_t)k] = s.kf_cap - 3; refused_p(d, kUlmRowStore, DVM_ERR_INVALID, "row of another store"); }
    if (n_kfs > 1) { Scene d = s; d.kf_slot[(size_t)k] = s.kf_slot[(size_t)((k + 1) % n_kfs)]; refused_p(d, kUlmKfTwice, DVM_ERR_INVALID, "kf_slot twice"); }
  }
  std::printf("n %d n_kfs %d ok\n", n, n_kfs);
}

int main() {
  const int sizes[] = {0, 1, 63, 64, 65, 257, 1025};
  const int kfs[] = {0, 1, 3, 9};
  unsigned seed = 1;
  for (size_t i = 0; i < 7; i++) call(sizes[i], kfs[i % 4], seed++);
  { UlmReserve R{32, 2048, 80, 100000, 2000, 2048}; EXPECT(ulm_check_reserve(R).fault == kUlmOk); }
  { UlmReserve R{1, 1, 1, 1, 1, 0}; EXPECT(ulm_check_reserve(R).fault == kUlmSizes); }
  { UlmReserve R{1, 1, 1 << 20, 1, 1, 8192}; EXPECT(ulm_check_reserve(R).fault == kUlmSizes); }   // keys would pass the idle word
  { UlmReserve R{1 << 16, 1, 1, 1 << 16, 1, 64}; EXPECT(ulm_check_reserve(R).fault == kUlmSizes); }
  { UlmReserve R{-1, 1, 1, 1, 1, 64}; EXPECT(ulm_check_reserve(R).fault == kUlmSizes); }
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("every verdict as the direct enumeration\n");
  return 0;
}
