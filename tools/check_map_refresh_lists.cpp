// tools/check_map_refresh_lists.cpp -- the host checks of dvm_map_store_refresh (dvm_slam_amd/csrc/map_refresh_lists.h) against a
// brute-force restatement: a call passes exactly when the direct enumeration finds no offence, a refused call names an offence the
// enumeration finds too, and after a pass every index the kernel forms -- obs_off[p] + j, obs.kf, obs.kp, the map slot, the ref -- lies
// inside its array.  Calls at n_points and N of 0, 1, 63, 64, 65 and 257, with bad keyframes with and without a slot, new points, and
// each offence planted in turn.  Plain g++, no HIP header (tests/test_map_refresh_lists.py builds it, also with sanitizers).
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../dvm_slam_amd/csrc/map_refresh_lists.h"

using namespace dvm;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Call {
  std::vector<int32_t> mp_slot, obs_off, ref_obs, best;
  std::vector<dvm_mp_obs> obs;
  std::vector<dvm_mp_refresh_kf> kfs;
  std::vector<MprKfMeta> meta;
  std::vector<uint8_t> is_new, written;
  std::vector<float> new_pos;
  std::vector<uint32_t> stamp;
  uint32_t gen = 0, what = DVM_MPR_DESCRIPTOR | DVM_MPR_GEOMETRY;
  int capacity = 0;
  bool with_new = true;
  dvm_mp_refresh view() const {
    dvm_mp_refresh in{};
    in.n_points = (int32_t)mp_slot.size(); in.n_kfs = (int32_t)kfs.size(); in.n_obs = (int32_t)obs.size(); in.what = what;
    in.mp_slot = mp_slot.data(); in.obs_off = obs_off.data(); in.obs = obs.data(); in.ref_obs = ref_obs.data(); in.kfs = kfs.data();
    in.is_new = with_new ? is_new.data() : nullptr; in.new_pos = with_new ? new_pos.data() : nullptr;
    in.best_obs_out = const_cast<int32_t*>(best.data());
    return in;
  }
  MprVerdict run() {
    const dvm_mp_refresh in = view();
    const MprVerdict a = mpr_check_args(in);
    if (a.fault != kMprOk) return a;
    return mpr_check_lists(in, capacity, written.data(), stamp.data(), ++gen, meta.data());
  }
};

// every offence of the call, by direct enumeration (no early exit, its own walk of the arrays)
static std::set<int> offences(const Call& c) {
  std::set<int> f;
  const int L = (int)c.mp_slot.size(), E = (int)c.obs.size(), K = (int)c.kfs.size();
  if (c.what == 0 || c.what > 3) f.insert(kMprWhat);
  bool off_ok = c.obs_off[0] == 0 && c.obs_off[(size_t)L] == E;
  for (int p = 0; p < L; p++) off_ok = off_ok && c.obs_off[(size_t)p + 1] >= c.obs_off[(size_t)p];
  if (!off_ok) { f.insert(kMprOff); return f; }                       // (nothing below can be indexed)
  auto gone = [&](int k) { return (c.kfs[(size_t)k].flags & 1u) && c.kfs[(size_t)k].slot == -1; };
  for (int k = 0; k < K; k++) {
    if (c.kfs[(size_t)k].flags > 1u) f.insert(kMprKfFlags);
    if (!gone(k) && c.meta[(size_t)k].n < 0) f.insert(kMprKfSlot);
  }
  for (int p = 0; p < L; p++) {
    const int sl = c.mp_slot[(size_t)p], o0 = c.obs_off[(size_t)p], N = c.obs_off[(size_t)p + 1] - o0;
    const bool fresh = c.with_new && c.is_new[(size_t)p];
    const bool in_store = sl >= 0 && sl < c.capacity;
    if (!in_store) f.insert(kMprMapSlot);
    for (int q = 0; q < p; q++) if (c.mp_slot[(size_t)q] == sl) f.insert(kMprMapTwice);
    if (in_store && !fresh && !c.written[(size_t)sl]) f.insert(kMprUnwritten);
    if (fresh && N == 0) f.insert(kMprNewEmpty);
    if (fresh && c.what != 3) f.insert(kMprNewWhat);
    if (N > 512) f.insert(kMprTooMany);
    for (int j = 0; j < N; j++) {
      const dvm_mp_obs ob = c.obs[(size_t)(o0 + j)];
      if (ob.kf < 0 || ob.kf >= K) { f.insert(kMprObsKf); continue; }
      if (!gone(ob.kf) && (ob.kp < 0 || ob.kp >= c.meta[(size_t)ob.kf].n)) f.insert(kMprKp);
    }
    if ((c.what & 2u) && N >= 1) {
      const int r = c.ref_obs[(size_t)p];
      if (r < 0 || r >= N) f.insert(kMprRef);
      else { const int k = c.obs[(size_t)(o0 + r)].kf; if (k >= 0 && k < K && gone(k)) f.insert(kMprRefBad); }
    }
  }
  return f;
}

static Call make(int L, int N, unsigned seed) {
  std::mt19937 rng(seed);
  Call c;
  const int K = 7;                                     // keyframe 5: bad with a slot; keyframe 6: bad, slot -1
  c.capacity = 3 * L + 5;
  c.written.assign((size_t)c.capacity, 0); c.stamp.assign((size_t)c.capacity, 0);
  for (int k = 0; k < K; k++) {
    c.kfs.push_back(dvm_mp_refresh_kf{k == 6 ? -1 : 2 * k, k >= 5 ? 1u : 0u, {0.f, 1.f, 2.f}});
    c.meta.push_back(MprKfMeta{k == 6 ? -1 : 40 + k, 8});
  }
  c.obs_off.push_back(0);
  for (int p = 0; p < L; p++) {
    const int n = p % 3 == 2 ? 0 : p % 3 == 1 ? N : (N + 1) / 2;  // lists of N, of half of it and empty ones
    c.mp_slot.push_back(c.capacity - 1 - 3 * p);
    const bool fresh = n > 0 && p % 4 == 1;
    c.is_new.push_back(fresh ? 1 : 0);
    if (!fresh) c.written[(size_t)c.mp_slot.back()] = 1;
    int ref = 0;
    for (int j = 0; j < n; j++) {
      const int k = (int)(rng() % (unsigned)K);
      c.obs.push_back(dvm_mp_obs{k, k == 6 ? 1000000 : (int32_t)(rng() % (unsigned)(40 + k))});   // (kp of a keyframe without a slot: anything)
      if (k != 6) ref = j;
    }
    if (n > 0 && c.obs[c.obs.size() - (size_t)n + (size_t)ref].kf == 6) c.obs[c.obs.size() - (size_t)n + (size_t)ref] = dvm_mp_obs{0, 0};
    c.ref_obs.push_back(ref);
    c.obs_off.push_back((int32_t)c.obs.size());
    for (int q = 0; q < 3; q++) c.new_pos.push_back(1.f);
  }
  c.best.assign((size_t)L + 1, 0);
  if (c.obs.empty()) c.obs.reserve(1);
  return c;
}

static unsigned rng_pick(int p) { return ((unsigned)p * 2654435761u) >> 7; }

static void expect_refused(Call c, int fault, int rc, const char* what) {
  const std::set<int> f = offences(c);
  const MprVerdict v = c.run();
  if (!(v.fault != kMprOk && f.count(v.fault) && f.count(fault) && v.rc() != DVM_OK && (v.fault != fault || v.rc() == rc))) {
    std::printf("FAILED: %s: verdict %d rc %d\n", what, v.fault, v.rc());
    fails++;
  }
}

static void call(int L, int N, unsigned seed) {
  Call c = make(L, N, seed);
  EXPECT(offences(c).empty());
  const MprVerdict v = c.run();
  EXPECT(v.fault == kMprOk && v.rc() == DVM_OK);
  int longest = 0;
  for (int p = 0; p < L; p++) {                        // what the kernel indexes with
    const int o0 = c.obs_off[(size_t)p], n = c.obs_off[(size_t)p + 1] - o0;
    longest = n > longest ? n : longest;
    EXPECT(o0 >= 0 && o0 + n <= (int)c.obs.size() && c.mp_slot[(size_t)p] >= 0 && c.mp_slot[(size_t)p] < c.capacity);
    for (int j = 0; j < n; j++) {
      const dvm_mp_obs ob = c.obs[(size_t)(o0 + j)];
      EXPECT(ob.kf >= 0 && ob.kf < (int)c.kfs.size());
      if (c.kfs[(size_t)ob.kf].slot >= 0) EXPECT(ob.kp >= 0 && ob.kp < c.meta[(size_t)ob.kf].n);
    }
    if (n) EXPECT(c.ref_obs[(size_t)p] >= 0 && c.ref_obs[(size_t)p] < n && c.kfs[(size_t)c.obs[(size_t)(o0 + c.ref_obs[(size_t)p])].kf].slot >= 0);
  }
  EXPECT(v.max_obs == longest);
  { Call d = c; d.what = DVM_MPR_DESCRIPTOR; d.with_new = false; for (int p = 0; p < L; p++) d.written[(size_t)d.mp_slot[(size_t)p]] = 1;
    for (auto& r : d.ref_obs) r = -7;                  // (not read without GEOMETRY)
    EXPECT(offences(d).empty() && d.run().fault == kMprOk); }
  // the call's own fields
  { Call d = c; d.what = 0; expect_refused(d, kMprWhat, DVM_ERR_INVALID, "what 0"); d.what = 4; expect_refused(d, kMprWhat, DVM_ERR_INVALID, "what 4"); }
  { Call d = c; dvm_mp_refresh in = d.view(); in.n_obs = -1; EXPECT(mpr_check_args(in).fault == kMprCounts); }
  { Call d = c; dvm_mp_refresh in = d.view();
    if (L) { in.new_pos = nullptr; EXPECT(mpr_check_args(in).fault == kMprNull); }      // (is_new without new_pos)
    in = d.view(); in.obs_off = nullptr; EXPECT(mpr_check_args(in).fault == kMprNull);
    if (L) { in = d.view(); in.best_obs_out = nullptr; EXPECT(mpr_check_args(in).fault == kMprNull); in = d.view(); in.ref_obs = nullptr; EXPECT(mpr_check_args(in).fault == kMprNull);
             in = d.view(); in.mp_slot = nullptr; EXPECT(mpr_check_args(in).fault == kMprNull); in = d.view(); in.kfs = nullptr; EXPECT(mpr_check_args(in).fault == kMprNull); }
    if (!c.obs.empty()) { in = d.view(); in.obs = nullptr; EXPECT(mpr_check_args(in).fault == kMprNull); } }
  // the CSR
  { Call d = c; d.obs_off[0] = 1; expect_refused(d, kMprOff, DVM_ERR_INVALID, "obs_off[0]"); }
  { Call d = c; d.obs_off[(size_t)L] += 1; expect_refused(d, kMprOff, DVM_ERR_INVALID, "obs_off[L] beyond n_obs"); }
  if (L >= 2 && c.obs_off[1] > 0) { Call d = c; d.obs_off[1] = d.obs_off[2] + 1; expect_refused(d, kMprOff, DVM_ERR_INVALID, "obs_off falls"); }
  // keyframe entries
  { Call d = c; d.kfs[2].flags = 2u; expect_refused(d, kMprKfFlags, DVM_ERR_INVALID, "unknown keyframe flags"); }
  { Call d = c; d.meta[3].n = -1; expect_refused(d, kMprKfSlot, DVM_ERR_INVALID, "keyframe slot never written"); }
  { Call d = c; d.kfs[0].slot = -1; d.meta[0].n = -1; expect_refused(d, kMprKfSlot, DVM_ERR_INVALID, "slot -1 on a keyframe that is not bad"); }
  for (int p = 0; p < L; p += (p >= 8 && p < L - 3 ? L / 7 : 1)) {     // (every point of a small call, a sample of a large one)
    const int o0 = c.obs_off[(size_t)p], n = c.obs_off[(size_t)p + 1] - o0;
    const bool fresh = c.is_new[(size_t)p] != 0;
    { Call d = c; d.mp_slot[(size_t)p] = d.capacity; expect_refused(d, kMprMapSlot, DVM_ERR_INVALID, "map slot = capacity"); d.mp_slot[(size_t)p] = -1; expect_refused(d, kMprMapSlot, DVM_ERR_INVALID, "map slot -1"); }
    if (p > 0) { Call d = c; d.mp_slot[(size_t)p] = d.mp_slot[0]; if (fresh) d.written[(size_t)d.mp_slot[0]] = 1; expect_refused(d, kMprMapTwice, DVM_ERR_INVALID, "map slot twice"); }
    if (!fresh) { Call d = c; d.written[(size_t)d.mp_slot[(size_t)p]] = 0; expect_refused(d, kMprUnwritten, DVM_ERR_INVALID, "old point never written"); }
    if (n == 0) { Call d = c; d.is_new[(size_t)p] = 1; expect_refused(d, kMprNewEmpty, DVM_ERR_INVALID, "new point without observations"); }
    if (fresh) { Call d = c; d.what = DVM_MPR_GEOMETRY; expect_refused(d, kMprNewWhat, DVM_ERR_INVALID, "new point, GEOMETRY only"); d.what = DVM_MPR_DESCRIPTOR; expect_refused(d, kMprNewWhat, DVM_ERR_INVALID, "new point, DESCRIPTOR only"); }
    if (n) {
      const size_t at = (size_t)(o0 + (int)(rng_pick(p) % (unsigned)n));
      { Call d = c; d.obs[at].kf = 7; expect_refused(d, kMprObsKf, DVM_ERR_INVALID, "kf = n_kfs"); d.obs[at].kf = -1; expect_refused(d, kMprObsKf, DVM_ERR_INVALID, "kf -1"); }
      { Call d = c; d.obs[at].kf = 2; d.obs[at].kp = 42; expect_refused(d, kMprKp, DVM_ERR_INVALID, "kp = n"); d.obs[at].kp = -1; expect_refused(d, kMprKp, DVM_ERR_INVALID, "kp -1"); }
      { Call d = c; d.ref_obs[(size_t)p] = n; expect_refused(d, kMprRef, DVM_ERR_INVALID, "ref = N"); d.ref_obs[(size_t)p] = -1; expect_refused(d, kMprRef, DVM_ERR_INVALID, "ref -1"); }
      { Call d = c; d.obs[(size_t)(o0 + d.ref_obs[(size_t)p])].kf = 6; expect_refused(d, kMprRefBad, DVM_ERR_INVALID, "ref on a keyframe without a slot"); }
      { Call d = c; d.obs[(size_t)(o0 + d.ref_obs[(size_t)p])] = dvm_mp_obs{5, 3}; EXPECT(offences(d).empty() && d.run().fault == kMprOk); }     // a bad keyframe WITH a slot may be the ref
    }
  }
  std::printf("L %d N %d ok\n", L, N);
}

int main() {
  const int sizes[] = {0, 1, 63, 64, 65, 257};
  unsigned seed = 1;
  for (int L : sizes)
    for (int N : sizes) call(L, N, seed++);
  {                                                    // the capacity limit: 512 passes, 513 is DVM_ERR_CAPACITY
    Call c = make(2, 512, 99);
    EXPECT(c.run().fault == kMprOk);
    Call d = make(2, 513, 99);
    const MprVerdict v = d.run();
    EXPECT(v.fault == kMprTooMany && v.rc() == DVM_ERR_CAPACITY && v.point == 1 && offences(d).count(kMprTooMany));
  }
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("every verdict as the direct enumeration\n");
  return 0;
}
