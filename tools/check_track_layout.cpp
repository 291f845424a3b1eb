// tools/check_track_layout.cpp -- the working-set layouts of dvm_tracker (dvm_slam_amd/csrc/track_layout.h) over a grid of
// (max_frames, max_keypoints, max_queries, max_points): every reserved size is the layout measured at the largest arguments and equals the
// hand-summed formula the reservations used before the layouts were written once (copied below as the expected value); every item starts at
// a multiple of its alignment, lies inside its block and overlaps no other; every smaller call shape the entry points can produce fits.
// The blocks are address space only (PROT_NONE): nothing is read or written.  Plain g++ with the HIP headers on the include path, no device
// library (tests/test_host_logic.py builds it, also with sanitizers: measuring on a null base must not do pointer arithmetic).
#include <sys/mman.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../dvm_slam_amd/csrc/track_layout.h"

using namespace dvm;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s  [B=%zu K=%zu Q=%zu P=%zu]\n", __FILE__, __LINE__, #c, g_B, g_K, g_Q, g_P); fails++; } } while (0)
static size_t g_B, g_K, g_Q, g_P;

struct Item { uintptr_t at; size_t bytes, align; };
#define ITEM(p, count) Item{reinterpret_cast<uintptr_t>(p), (size_t)(count) * sizeof(*(p)), alignof(decltype(*(p)))}

// address space for a block of `bytes` (page aligned, so every 256-byte item boundary of the block is one of the address too)
struct Space {
  uint8_t* base; size_t bytes;
  explicit Space(size_t n) : bytes(std::max<size_t>(n, 1)) {
    void* p = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    base = p == MAP_FAILED ? nullptr : static_cast<uint8_t*>(p);
  }
  ~Space() { if (base) munmap(base, bytes); }
};

// items aligned, inside [base, base + bytes), pairwise disjoint
static void check_items(const uint8_t* base, size_t bytes, std::vector<Item> items) {
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base);
  std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.at < b.at; });
  for (size_t i = 0; i < items.size(); i++) {
    const Item& it = items[i];
    EXPECT(it.at % it.align == 0);
    EXPECT(it.at >= lo && it.at + it.bytes <= lo + bytes);
    if (i) EXPECT(items[i - 1].at + items[i - 1].bytes <= it.at);
  }
}

static std::vector<Item> items_of(const QueryBlock& m, size_t count, size_t Qs) {
  const size_t Qn = count * Qs;
  return {ITEM(m.qdesc, Qn * 32), ITEM(m.qx, Qn), ITEM(m.qy, Qn), ITEM(m.qr, Qn), ITEM(m.qmin, Qn), ITEM(m.qmax, Qn), ITEM(m.q_claims, Qn), ITEM(m.q_angle, Qn),
          ITEM(m.q_pos, Qn * 3), ITEM(m.pose_in, count * 7), ITEM(m.nq_arr, count), ITEM(m.inv_sigma2, 64)};
}
static std::vector<Item> items_of(const ResidentUpload& u, size_t count, size_t E) {
  return {ITEM(u.scale, 64), ITEM(u.inv_sigma2, 64), ITEM(u.fr, count), ITEM(u.slot, E), ITEM(u.angle, E), ITEM(u.octave, E)};
}
static std::vector<Item> items_of(const LocalMapUpload& u, size_t count, size_t T, size_t ks) {
  return {ITEM(u.scale, 64), ITEM(u.inv_sigma2, 64), ITEM(u.pose, count * 7), ITEM(u.fa, count), ITEM(u.qoff, count), ITEM(u.skip_on, count), ITEM(u.pts, T),
          ITEM(u.frame_mp, count * ks)};
}
static std::vector<Item> items_of(const LocalMapWork& w, size_t count, size_t T, size_t ocap) {
  const LocalQueries& q = w.LQ;
  const size_t Kb = count * ocap;
  return {ITEM(q.seen, T), ITEM(q.pos, T * 3), ITEM(q.claims, T), ITEM(q.frame_mp, Kb), ITEM(q.skip, Kb), ITEM(q.pose_in, count * 7), ITEM(q.qdesc, T * 32),
          ITEM(q.qx, T), ITEM(q.qy, T), ITEM(q.qr, T), ITEM(q.qmin, T), ITEM(q.qmax, T), ITEM(q.q_claims, T), ITEM(q.q_tab, T), ITEM(w.ranked, T * 4),
          ITEM(w.lres, count * 8), ITEM(q.nq, count * 8)};
}

static size_t p256(size_t b) { return pad<256>(b); }

static void check(size_t B, size_t K, size_t max_queries, size_t max_points) {
  const size_t Q = (max_queries + 63) & ~(size_t)63, P = (max_points + 63) & ~(size_t)63;
  g_B = B; g_K = K; g_Q = Q; g_P = P;
  const size_t kp = sizeof(dvm_keypoint_pod);

  // ---- dvm_tracker_create_batch: the formulas it summed by hand
  const size_t want_d = p256(B * Q * 16) + p256(B * K * 4) + p256(B * 32) + p256(B * K * 24) + p256(B * K * 16) + 2 * p256(B * K * 8) + p256(B * K * 4) + p256(B * 4) +
                        p256(B * K) + p256(B * K * kp);
  const size_t want_q = p256(B * Q * 32) + 3 * p256(B * Q * 4) + 2 * p256(B * Q * 4) + p256(B * Q) + p256(B * Q * 4) + p256(B * Q * 12) + p256(B * 56) + p256(B * 4) +
                        p256(64 * 4);
  const size_t want_m = want_q + p256(B * K * 4) + p256(B * K) + p256(B * 32) + p256(B * 16) + p256(B * 4) + p256(B * 56) + p256(B * 4) + p256(K * kp);
  const size_t want_rup = p256(2 * 256 + pad<64>(B * sizeof(ResidentFrame)) + B * Q * 9);
  const size_t want_rm = want_rup + p256(B * Q * 4) + p256(B * 4);
  const size_t q_bytes = carve_query_block(nullptr, B, Q).bytes;
  EXPECT(q_bytes == want_q);
  EXPECT(carve_tracker_device(nullptr, B, K, Q, q_bytes).bytes == want_d + want_q);
  EXPECT(q_bytes + carve_tracker_results(nullptr, B, K).bytes == want_m);
  const ResidentMapped rms = carve_resident_mapped(nullptr, B, Q);
  EXPECT(rms.up == want_rup && rms.bytes == want_rm);
  EXPECT(rms.entry == nullptr && rms.nq == nullptr);           // measuring forms no address
  {   // the device block
    Space sp(want_d + want_q);
    const TrackerDevice d = carve_tracker_device(sp.base, B, K, Q, q_bytes);
    EXPECT(d.bytes == sp.bytes);
    check_items(sp.base, sp.bytes, {ITEM(d.ranked, B * Q * 4), ITEM(d.assign, B * K), ITEM(d.res, B * 8), ITEM(d.Xw, B * K * 3), ITEM(d.obs, B * K * 2), ITEM(d.info, B * K),
                                    ITEM(d.chi, B * K), ITEM(d.edge_kp, B * K), ITEM(d.nedges, B), ITEM(d.edge_out, B * K), ITEM(d.kps_un, B * K), ITEM(d.q, q_bytes)});
  }
  {   // the mapped block: [query block of any call][results]
    Space sp(want_m);
    const TrackerResults m = carve_tracker_results(sp.base + q_bytes, B, K);
    std::vector<Item> res = {ITEM(m.assign, B * K), ITEM(m.outlier, B * K), ITEM(m.res, B * 8), ITEM(m.fin, B * 4), ITEM(m.nedges, B), ITEM(m.pose_out, B * 7),
                             ITEM(m.n_inl, B), ITEM(m.kps_un, K)};
    check_items(sp.base + q_bytes, m.bytes, res);
    // every call shape finish_run accepts: count <= B frames at a stride that is a multiple of 64 with count * Qs <= B * Q
    for (size_t count : {(size_t)1, (B + 1) / 2, B})
      for (size_t Qs = 64; Qs <= Q; Qs += 64) {                       // every stride finish_run can choose
        const QueryBlock qb = carve_query_block(sp.base, count, Qs);
        EXPECT(qb.bytes <= q_bytes);
        std::vector<Item> all = items_of(qb, count, Qs);
        all.insert(all.end(), res.begin(), res.end());
        check_items(sp.base, sp.bytes, all);
      }
    const QueryBlock top = carve_query_block(sp.base, B, Q);
    EXPECT(top.bytes == q_bytes);
    check_items(sp.base, q_bytes, items_of(top, B, Q));
  }
  {   // the resident first half: uploads of count frames whose lists (each rounded up to 64) sum to E <= count * Q
    Space sp(want_rm);
    const ResidentMapped rm = carve_resident_mapped(sp.base, B, Q);
    EXPECT(rm.up == want_rup && rm.bytes == want_rm);
    const std::vector<Item> tail = {ITEM(rm.entry, B * Q), ITEM(rm.nq, B)};
    for (size_t count : {(size_t)1, (B + 1) / 2, B})
      for (size_t E : {(size_t)0, (size_t)64, count * Q / 2 / 64 * 64, count * Q}) {
        const ResidentUpload u = carve_resident_upload(sp.base, count, E);
        EXPECT(u.bytes <= rm.up);
        std::vector<Item> all = items_of(u, count, E);
        all.insert(all.end(), tail.begin(), tail.end());
        check_items(sp.base, sp.bytes, all);
      }
  }

  // ---- dvm_tracker_reserve_local_map
  const size_t kFrameRec = 7 * 8 + sizeof(LocalFrameArgs) + 8;
  const size_t want_up = p256(B * kFrameRec) + 2 * p256(256) + p256(P * sizeof(LocalPointPod)) + p256(B * K * 4) + p256(P * 4) + p256(B * 8);
  const size_t want_ld = want_up + p256(P) + p256(P * 12) + p256(P) + p256(B * K * 4) + p256(B * K) + p256(B * 56) + p256(P * 32) + 5 * p256(P * 4) + p256(P) + p256(P * 4) +
                         p256(P * 16) + 2 * p256(B * 32);
  const size_t want_lm = want_up + p256(B * K * 4) + p256(B * K) + p256(P * sizeof(TrackPoint)) + p256(B * 64) + p256(B * 56) + 3 * p256(B * 16);
  const size_t up = local_map_upload_capacity(B, P, K);
  const size_t work = carve_local_map_work(nullptr, B, P, K).bytes;
  EXPECT(up == want_up);
  EXPECT(up + work == want_ld);
  EXPECT(up + carve_local_map_results(nullptr, B, K, P).bytes == want_lm);
  {
    Space sp(want_ld);
    for (size_t count : {(size_t)1, (B + 1) / 2, B})
      for (size_t ocap : {(size_t)1, (K + 1) / 2, K})
        for (size_t T : {(size_t)64, std::max<size_t>(64, P / 2 / 64 * 64), P}) {
          const LocalMapWork W = carve_local_map_work(sp.base + up, count, T, ocap);
          EXPECT(W.bytes <= work);
          const std::vector<Item> wi = items_of(W, count, T, ocap);
          // the record form
          const LocalMapUpload u = carve_local_map_upload(sp.base, count, T, ocap);
          EXPECT(u.bytes <= up);
          std::vector<Item> all = items_of(u, count, T, ocap);
          all.insert(all.end(), wi.begin(), wi.end());
          check_items(sp.base, sp.bytes, all);
          // the resident form: what is copied up ends before the device-only tables
          const LocalMapUploadResident r = carve_local_map_upload_resident(sp.base, count, T, ocap);
          EXPECT(r.u.bytes <= up && r.copy_bytes <= r.u.bytes);
          EXPECT(reinterpret_cast<uintptr_t>(r.u.frame_mp) + count * ocap * 4 == reinterpret_cast<uintptr_t>(sp.base) + r.copy_bytes);
          EXPECT(reinterpret_cast<uintptr_t>(r.u.pts) >= reinterpret_cast<uintptr_t>(sp.base) + r.copy_bytes);
          all = items_of(r.u, count, T, ocap);
          all.push_back(ITEM(r.stores, count)); all.push_back(ITEM(r.slots, T));
          all.insert(all.end(), wi.begin(), wi.end());
          check_items(sp.base, sp.bytes, all);
          // both forms begin with the same head
          EXPECT(r.u.scale == u.scale && r.u.inv_sigma2 == u.inv_sigma2 && r.u.pose == u.pose && r.u.fa == u.fa && r.u.qoff == u.qoff && r.u.skip_on == u.skip_on);
        }
  }
  {
    Space sp(want_lm);
    const LocalMapResults r = carve_local_map_results(sp.base + up, B, K, P);
    check_items(sp.base + up, r.bytes, {ITEM(r.mp, B * K), ITEM(r.outlier, B * K), ITEM(r.tp, P), ITEM(r.res, B * 16), ITEM(r.pose, B * 7), ITEM(r.n_inl, B * 4),
                                        ITEM(r.fin, B * 4), ITEM(r.nedges, B * 4)});
    EXPECT(up + r.bytes == sp.bytes);
  }

  // ---- the reference-keyframe working set (R = P here): measured on a null base as well, and every smaller call inside
  const size_t kup = carve_keyframe_upload(nullptr, B, P).bytes;
  for (size_t count : {(size_t)1, (B + 1) / 2, B})
    for (size_t T : {(size_t)64, P}) EXPECT(carve_keyframe_upload(nullptr, count, T).bytes <= kup);
  {
    Space sp(carve_refkf_work(nullptr, B, K).bytes);
    const RefKfWork w = carve_refkf_work(sp.base, B, K);
    EXPECT(w.bytes == sp.bytes);
    check_items(sp.base, sp.bytes, {ITEM(w.word, B * K), ITEM(w.node, B * K), ITEM(w.w, B * K), ITEM(w.fv_node, B * K), ITEM(w.fv_feat, B * K), ITEM(w.fv_off, B * (K + 1)),
                                    ITEM(w.cnt, B * kRefKfCnt), ITEM(w.match, B * K), ITEM(w.bin, B * K)});
    EXPECT(carve_refkf_results(nullptr, B, K).bytes > 0 && carve_refkf_results(nullptr, B, K).pose == nullptr);
  }
}

int main() {
  const size_t grid[][4] = {{1, 1, 1, 1},          {1, 1000, 1000, 65},    {3, 4256, 4256, 3001}, {32, 1000, 1000, 96000}, {256, 8192, 8192, (size_t)1 << 20},
                            {2, 100, 65, 129},     {7, 1000, 999, 5000},   {1, 2048, 64, 64},     {5, 63, 127, 63}};
  for (const auto& g : grid) check(g[0], g[1], g[2], g[3]);
  if (fails) return 1;
  std::printf("track layout: %zu grid points, every size as reserved before\n", sizeof(grid) / sizeof(grid[0]));
  return 0;
}
