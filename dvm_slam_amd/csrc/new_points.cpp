// dvm_slam_amd/csrc/new_points.cpp -- dvm_new_points: LocalMapping::CreateNewMapPoints for all neighbours of a keyframe as one chain
// (include/dvmslam_hip.h; kernels in new_points_kernels.hip; the handle's stream, working set, packing cursor and kernel times: chain.h).
// The working set: a device block [packed upload][speculative results] and a mapped block [upload staging][results].  A call validates everything, packs both
// keyframe sets back to back into the staging region, sends it with ONE copy, queues the three launches, synchronises ONCE and copies the
// records out of the mapped block.  Host arithmetic here is index-free: the baseline test of each neighbour and the 3x4 pose matrices.
// dvm_create_new_map_points_resident: the keyframes are slots of a dvm_keyframe_store (keyframe_store.h).  The same body runs with every
// NpKfDev pointing into the store except mp, which is packed and sent as before; the launches are bracketed by kfs_read_begin / _end.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "chain.h"
#include "keyframe_store.h"
#include "new_points_kernels.h"
#include "orb_pipeline.h"
#include "camera_model.h"
#include "pose_f32.h"

using namespace dvm;

struct dvm_new_points : Chain {                 // ws: device block [up_bytes][spec]; mapped block [up_bytes][results]
  int max_n1 = 0, max_nb = 0, max_total = 0;
  size_t rec_cap = 0;                           // records the mapped block holds: max_nb * max_n1
  float last_ms[3] = {0, 0, 0};
  int64_t up_bytes_last = 0;                    // host-to-device bytes queued by the last call that reached the device
};

namespace {
using Cursor64 = Cursor<64>;                    // every item of the upload and of the results starts at a multiple of 64 bytes
// bytes a keyframe of n keypoints takes in the packed upload at most: per keypoint its cv::KeyPoint, descriptor, map point, and -- fv_n <= n
// nodes, at most n features -- a node id, an offset and a feature; per keyframe the last offset, two level tables of 64 and the rounding of
// its eight arrays.  Linear in n, so the neighbours' sum is bounded by their total.
constexpr size_t kKfPerKeypoint = sizeof(dvm_keypoint_pod) + 32 + 4 * 4, kKfFixed = 4 + 2 * 64 * 4 + 8 * 64;

int fail(int rc, const std::string& msg) { set_error("dvm_create_new_map_points: " + msg); return rc; }

// view != null: the keyframe lives in a store slot -- its arrays, FeatureVector and tables were checked when it was put; mp travels
int check_keyframe(const dvm_np_keyframe& k, const char* who, int n_levels, const KfSlotView* view = nullptr) {
  const std::string w(who);
  if (k.n < 0 || k.n > kFrameCap) return fail(DVM_ERR_INVALID, w + ": n outside [0, 8192]");
  if (k.n_levels != n_levels) return fail(DVM_ERR_INVALID, w + ": level tables of another length than the current keyframe's");
  if (view) {
    if (!(k.fx != 0.0f) || !(k.fy != 0.0f)) return fail(DVM_ERR_INVALID, w + ": zero focal length");
    if (k.n > 0 && !k.mp) return fail(DVM_ERR_INVALID, w + ": missing keypoint array");
    return DVM_OK;
  }
  if (!k.scale_factors || !k.level_sigma2) return fail(DVM_ERR_INVALID, w + ": missing level table");
  if (!(k.fx != 0.0f) || !(k.fy != 0.0f)) return fail(DVM_ERR_INVALID, w + ": zero focal length");
  if (k.n > 0 && (!k.kps || !k.desc || !k.mp)) return fail(DVM_ERR_INVALID, w + ": missing keypoint array");
  if (k.fv_n < 0 || k.fv_n > k.n) return fail(DVM_ERR_INVALID, w + ": more FeatureVector nodes than keypoints");
  if (k.fv_n > 0) {
    if (!k.fv_node || !k.fv_off || !k.fv_feat) return fail(DVM_ERR_INVALID, w + ": missing FeatureVector array");
    if (k.fv_off[0] != 0) return fail(DVM_ERR_INVALID, w + ": FeatureVector offsets do not start at 0");
    for (int a = 0; a < k.fv_n; a++) {
      if (k.fv_off[a + 1] < k.fv_off[a]) return fail(DVM_ERR_INVALID, w + ": FeatureVector offsets not monotone");
      if (a > 0 && (uint32_t)k.fv_node[a] <= (uint32_t)k.fv_node[a - 1])
        return fail(DVM_ERR_INVALID, w + ": FeatureVector nodes not ascending (as unsigned: node -1 is last)");
    }
    const int nf = k.fv_off[k.fv_n];
    if (nf > k.n) return fail(DVM_ERR_INVALID, w + ": more FeatureVector features than keypoints");
    for (int f = 0; f < nf; f++)
      if (k.fv_feat[f] < 0 || k.fv_feat[f] >= k.n) return fail(DVM_ERR_INVALID, w + ": FeatureVector feature index out of range");
  }
  return DVM_OK;
}

// packs one keyframe at the cursor (staging block -> device block) and returns its device view; of a keyframe in a store slot
// (view != null) only mp is packed, the other arrays are the slot's
NpKfDev pack_keyframe(const dvm_np_keyframe& k, Cursor64& c, const KfSlotView* view = nullptr) {
  NpKfDev v{};
  if (view) {
    v.kps = view->kps; v.desc = view->desc;
    v.mp = reinterpret_cast<const int32_t*>(c.put(k.mp, (size_t)k.n * 4));
    v.fv_node = view->fv_node; v.fv_off = view->fv_off; v.fv_feat = view->fv_feat;
    v.sf = view->sf; v.sigma2 = view->sigma2;
    v.n = k.n; v.fv_n = k.fv_n;
    return v;
  }
  const size_t n = (size_t)k.n, nf = k.fv_n > 0 ? (size_t)k.fv_off[k.fv_n] : 0;
  v.kps = reinterpret_cast<const dvm_keypoint_pod*>(c.put(k.kps, n * sizeof(dvm_keypoint_pod)));
  v.desc = c.put(k.desc, n * 32);
  v.mp = reinterpret_cast<const int32_t*>(c.put(k.mp, n * 4));
  v.fv_node = reinterpret_cast<const int32_t*>(c.put(k.fv_node, (size_t)k.fv_n * 4));
  v.fv_off = reinterpret_cast<const int32_t*>(c.put(k.fv_off, k.fv_n > 0 ? ((size_t)k.fv_n + 1) * 4 : 0));
  v.fv_feat = reinterpret_cast<const int32_t*>(c.put(k.fv_feat, nf * 4));
  v.sf = reinterpret_cast<const float*>(c.put(k.scale_factors, (size_t)k.n_levels * 4));
  v.sigma2 = reinterpret_cast<const float*>(c.put(k.level_sigma2, (size_t)k.n_levels * 4));
  v.n = k.n; v.fv_n = k.fv_n;
  return v;
}

// KeyFrame::GetPose().matrix3x4(), row-major (the rotation matrix of the unit quaternion | translation)
void pose_3x4(const dvm_se3f& T, float* out) {
  float R[9];
  dvm_pose::quat_matrix(T.q, R);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) out[4 * r + c] = R[3 * r + c];
    out[4 * r + 3] = T.t[r];
  }
}
}  // namespace

extern "C" {

int dvm_new_points_create(int device, dvm_new_points** out) { return chain_create(device, out); }
void dvm_new_points_destroy(dvm_new_points* h) { chain_destroy(h); }

int dvm_new_points_reserve(dvm_new_points* h, int max_kf1_keypoints, int max_neighbours, int max_total_neighbour_keypoints) {
  if (!h || max_kf1_keypoints < 0 || max_kf1_keypoints > kFrameCap || max_neighbours < 0 || max_total_neighbour_keypoints < 0 ||
      (int64_t)max_total_neighbour_keypoints > (int64_t)max_neighbours * kFrameCap) {
    set_error("dvm_new_points_reserve: bad sizes");
    return DVM_ERR_INVALID;
  }
  if (max_kf1_keypoints <= h->max_n1 && max_neighbours <= h->max_nb && max_total_neighbour_keypoints <= h->max_total) return DVM_OK;
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));
  const int n1 = std::max(max_kf1_keypoints, h->max_n1), nb = std::max(max_neighbours, h->max_nb), tot = std::max(max_total_neighbour_keypoints, h->max_total);
  h->max_n1 = h->max_nb = h->max_total = 0; h->rec_cap = 0;       // (a failed allocation leaves the handle holding nothing)
  const size_t n1p = ((size_t)n1 + 63) & ~(size_t)63;
  // (a KannalaBrandt8 call adds its per-neighbour geometry to the upload)
  const size_t up = pad<64>(((size_t)n1 + (size_t)tot) * kKfPerKeypoint + ((size_t)nb + 1) * kKfFixed + pad<64>((size_t)nb * sizeof(NpNbDev)) +
                            pad<64>((size_t)nb * sizeof(TriGeomKB8)));
  const size_t spec = (size_t)nb * n1p * 20 + 64;
  const size_t rec = (size_t)nb * (size_t)n1;
  const size_t res = pad<64>(((size_t)nb + 1) * 4) * 2 + pad<64>(rec * 8) + pad<64>(rec * 4) + pad<64>(rec * 12) + pad<64>((size_t)n1 * 4) + 64;
  if (const char* what = h->ws.alloc(up + spec, up + res, up, /*mapped*/ true, /*zeroed*/ false)) {
    set_error(std::string("dvm_new_points_reserve: ") + what + " failed");
    return DVM_ERR_HIP;
  }
  h->max_n1 = n1; h->max_nb = nb; h->max_total = tot; h->rec_cap = rec;
  return DVM_OK;
}

int dvm_new_points_profiling(dvm_new_points* h, int enable) {
  if (!h) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(h->device));
  return h->timer.enable(enable != 0);
}
int dvm_new_points_last_kernel_ms(dvm_new_points* h, float* ms) {
  if (!h || !ms) return DVM_ERR_INVALID;
  for (int i = 0; i < 3; i++) ms[i] = h->last_ms[i];
  return DVM_OK;
}
int dvm_new_points_last_upload_bytes(const dvm_new_points* h, int64_t* bytes) {
  if (!h || !bytes) return DVM_ERR_INVALID;
  *bytes = h->up_bytes_last;
  return DVM_OK;
}

}  // extern "C"

namespace {
// dvm_create_new_map_points and dvm_create_new_map_points_cam: kb8 == false runs the pinhole kernels on the keyframes' intrinsics; otherwise
// cur_model / nb_models / nb_poses (validated by the caller) go to the KannalaBrandt8 kernels.  store != null is
// dvm_create_new_map_points_resident: cur_view / nb_views[j] are the keyframes' slots, and of cur / nbs[j].kf the array pointers other
// than mp are not read (their counts, intrinsics and n_levels are the slots')
int create_new_map_points_impl(dvm_new_points* h, const dvm_np_keyframe* cur, int n_neighbours, const dvm_np_neighbour* nbs, const dvm_np_params* p,
                               dvm_np_out* out, bool kb8, const dvm_camera_model* cur_model, const dvm_camera_model* nb_models,
                               const dvm_pair_pose* nb_poses, const dvm_keyframe_store* store = nullptr, const KfSlotView* cur_view = nullptr,
                               const KfSlotView* nb_views = nullptr) {
  static_assert(sizeof(dvm_keypoint) == sizeof(dvm_keypoint_pod), "layout");
  if (!h || !cur || !p || !out || n_neighbours < 0 || (n_neighbours > 0 && !nbs)) return fail(DVM_ERR_INVALID, "missing argument");
  if (p->monocular != 1) return fail(DVM_ERR_INVALID, "only monocular keyframes (the stereo branches are outside the accelerated path)");
  if (!out->nb_status || !out->nb_matches || !out->pair_off || (cur->n > 0 && !out->new_point) || out->record_cap < 0 ||
      (out->record_cap > 0 && (!out->pairs || !out->status || !out->x3D)))
    return fail(DVM_ERR_INVALID, "missing output array");
  if (cur->n_levels < 1 || cur->n_levels > 64) return fail(DVM_ERR_INVALID, "n_levels outside [1, 64]");
  int rc = check_keyframe(*cur, "current keyframe", cur->n_levels, cur_view);
  if (rc != DVM_OK) return rc;
  int64_t total = 0;
  for (int j = 0; j < n_neighbours; j++) {
    rc = check_keyframe(nbs[j].kf, ("neighbour " + std::to_string(j)).c_str(), cur->n_levels, store ? &nb_views[j] : nullptr);
    if (rc != DVM_OK) return rc;
    total += nbs[j].kf.n;
  }
  if (cur->n > h->max_n1 || n_neighbours > h->max_nb || total > h->max_total)
    return fail(DVM_ERR_CAPACITY, "beyond the reservation (dvm_new_points_reserve): " + std::to_string(cur->n) + " keypoints, " + std::to_string(n_neighbours) +
                                      " neighbours with " + std::to_string(total) + " keypoints");
  int64_t nq0 = 0;
  for (int i = 0; i < cur->n; i++) nq0 += cur->mp[i] < 0 ? 1 : 0;
  if ((int64_t)out->record_cap < nq0 * n_neighbours) return fail(DVM_ERR_CAPACITY, "record_cap below n_neighbours x keypoints without a point");

  // the baseline test (LocalMapping.cc:497-512), float, one operation per statement
  std::vector<int> run;
  for (int j = 0; j < n_neighbours; j++) {
    const float dx = nbs[j].kf.Ow[0] - cur->Ow[0], dy = nbs[j].kf.Ow[1] - cur->Ow[1], dz = nbs[j].kf.Ow[2] - cur->Ow[2];
    float s = dx * dx;
    const float yy = dy * dy, zz = dz * dz;
    s = s + yy;
    s = s + zz;
    const float baseline = sqrtf(s);
    const float ratio = baseline / nbs[j].median_depth;
    const bool skip = (double)ratio < 0.01;
    out->nb_status[j] = skip ? 1 : 0;
    out->nb_matches[j] = 0;
    if (!skip) run.push_back(j);
  }
  const int nrun = (int)run.size(), n1 = cur->n;
  const size_t n1p = ((size_t)n1 + 63) & ~(size_t)63;
  for (int i = 0; i < n1; i++) out->new_point[i] = -1;
  for (int j = 0; j <= n_neighbours; j++) out->pair_off[j] = 0;
  if (nrun == 0 || n1 == 0) return DVM_OK;

  DVM_HIP(hipSetDevice(h->device));
  // pack: [NpNbDev x nrun][current keyframe][neighbours that run]
  WorkingSet& ws = h->ws;
  Cursor64 up{ws.hm, ws.d};
  NpNbDev* nb_stage = up.carve<NpNbDev>((size_t)nrun);
  const size_t gk_off = up.used();
  TriGeomKB8* gk_stage = kb8 ? up.carve<TriGeomKB8>((size_t)nrun) : nullptr;
  NpArgs A{};
  A.cur = pack_keyframe(*cur, up, cur_view);
  float T1w[12];
  pose_3x4(cur->Tcw, T1w);
  for (int r = 0; r < nrun; r++) {
    const dvm_np_neighbour& nb = nbs[run[r]];
    NpNbDev& D = nb_stage[r];
    std::memset(&D, 0, sizeof(D));
    D.kf = pack_keyframe(nb.kf, up, store ? &nb_views[run[r]] : nullptr);
    TriPair& P = D.P;
    P.cos_parallax_max = p->cos_parallax_max;
    P.K1[0] = cur->fx; P.K1[1] = cur->fy; P.K1[2] = cur->cx; P.K1[3] = cur->cy;
    P.K2[0] = nb.kf.fx; P.K2[1] = nb.kf.fy; P.K2[2] = nb.kf.cx; P.K2[3] = nb.kf.cy;
    std::memcpy(P.T1w, T1w, sizeof(T1w));
    pose_3x4(nb.kf.Tcw, P.T2w);
    std::memcpy(P.Ow1, cur->Ow, 12); std::memcpy(P.Ow2, nb.kf.Ow, 12);
    P.ratio_factor = p->ratio_factor; P.th_far = p->th_far; P.far_points = p->far_points ? 1 : 0; P.n_levels = cur->n_levels;
    std::memcpy(D.G.F12, nb.F12, 36); D.G.ep[0] = nb.ep[0]; D.G.ep[1] = nb.ep[1];
    D.G.coarse = p->coarse != 0; D.G.th_low = 50;   // ORBmatcher::TH_LOW
    if (kb8) {
      TriGeomKB8& GK = gk_stage[r];
      GK.ep[0] = nb.ep[0]; GK.ep[1] = nb.ep[1];
      GK.coarse = D.G.coarse; GK.th_low = D.G.th_low;
      std::memcpy(&GK.R, &nb_poses[run[r]], sizeof(GK.R));
      std::memcpy(GK.cam1, cur_model->p, 32); std::memcpy(GK.cam2, nb_models[run[r]].p, 32);
    }
  }
  if (up.used() > ws.up_bytes) return fail(DVM_ERR_CAPACITY, "packed keyframes exceed the reserved upload region");   // (cannot happen: kKfPerKeypoint / kKfFixed bound every keyframe)
  A.nb = reinterpret_cast<const NpNbDev*>(ws.d);
  A.nrun = nrun; A.n1 = n1; A.n1p = (int32_t)n1p; A.nfeat1 = cur_view ? cur_view->n_feat : cur->fv_n > 0 ? cur->fv_off[cur->fv_n] : 0;
  A.n_levels = cur->n_levels; A.check_ori = p->check_ori != 0;
  uint8_t* spec = ws.d + ws.up_bytes;
  A.best = reinterpret_cast<int32_t*>(spec);
  A.st = A.best + (size_t)nrun * n1p;
  A.X = reinterpret_cast<float*>(A.st + (size_t)nrun * n1p);
  // results in the mapped block (sized for the reservation)
  Cursor64 res{ws.hm + ws.up_bytes};
  int32_t* r_matches = res.carve<int32_t>((size_t)h->max_nb + 1);
  int32_t* r_off = res.carve<int32_t>((size_t)h->max_nb + 1);
  int32_t* r_pairs = res.carve<int32_t>(h->rec_cap * 2);
  int32_t* r_status = res.carve<int32_t>(h->rec_cap);
  float* r_x3D = res.carve<float>(h->rec_cap * 3);
  int32_t* r_new = res.carve<int32_t>((size_t)h->max_n1);
  A.h_matches = ws.dev(r_matches); A.h_pair_off = ws.dev(r_off); A.h_pairs = ws.dev(r_pairs); A.h_status = ws.dev(r_status); A.h_x3D = ws.dev(r_x3D);
  A.h_new_point = ws.dev(r_new);

  DVM_HIP(hipMemcpyAsync(ws.d, ws.hm, up.used(), hipMemcpyHostToDevice, h->s));
  h->up_bytes_last = (int64_t)up.used();
  DVM_HIP(hipMemsetAsync(A.best, 0xFF, (size_t)nrun * n1p * 4, h->s));
  if (store) { rc = kfs_read_begin(store, h->s); if (rc != DVM_OK) return rc; }
  const EventTimer& tm = h->timer;
  DVM_HIP(tm.mark(0, h->s));
  if (kb8) {
    NpArgsKB8 K{};
    K.A = A;
    K.G = reinterpret_cast<const TriGeomKB8*>(ws.d + gk_off);
    launch_np_search_kb8(h->s, K);
    DVM_HIP(tm.mark(1, h->s));
    launch_np_geometry_kb8(h->s, K);
  } else {
    launch_np_search(h->s, A);
    DVM_HIP(tm.mark(1, h->s));
    launch_np_geometry(h->s, A);
  }
  DVM_HIP(tm.mark(2, h->s));
  launch_np_settle(h->s, A);
  DVM_HIP(tm.mark(3, h->s));
  if (store) { rc = kfs_read_end(store, h->s); if (rc != DVM_OK) return rc; }
  rc = hip_check(hipGetLastError(), "dvm_create_new_map_points launch");
  const int rs = hip_check(hipStreamSynchronize(h->s), "dvm_create_new_map_points sync");
  if (rc != DVM_OK) return rc;
  if (rs != DVM_OK) return rs;
  if (tm.on)
    for (int i = 0; i < 3; i++) DVM_HIP(tm.elapsed(i, i + 1, &h->last_ms[i]));

  const size_t nrec = (size_t)r_off[nrun];
  if (nrec > (size_t)out->record_cap || nrec > h->rec_cap) return fail(DVM_ERR_STATE, "more records than the bound allows");   // (an internal error)
  for (int r = 0; r < nrun; r++) out->nb_matches[run[r]] = r_matches[r];
  for (int j = 0, r = 0; j < n_neighbours; j++) {     // a skipped neighbour's range is empty
    out->pair_off[j] = r_off[r];
    if (r < nrun && run[r] == j) r++;
  }
  out->pair_off[n_neighbours] = (int32_t)nrec;
  if (nrec) {
    std::memcpy(out->pairs, r_pairs, nrec * 8);
    std::memcpy(out->status, r_status, nrec * 4);
    std::memcpy(out->x3D, r_x3D, nrec * 12);
  }
  std::memcpy(out->new_point, r_new, (size_t)n1 * 4);
  return DVM_OK;
}
}  // namespace

extern "C" {

int dvm_create_new_map_points(dvm_new_points* h, const dvm_np_keyframe* cur, int n_neighbours, const dvm_np_neighbour* nbs,
                              const dvm_np_params* p, dvm_np_out* out) {
  return create_new_map_points_impl(h, cur, n_neighbours, nbs, p, out, false, nullptr, nullptr, nullptr);
}

int dvm_create_new_map_points_cam(dvm_new_points* h, const dvm_np_keyframe* cur, const dvm_camera_model* cur_model, int n_neighbours,
                                  const dvm_np_neighbour* nbs, const dvm_camera_model* nb_models, const dvm_pair_pose* nb_poses,
                                  const dvm_np_params* p, dvm_np_out* out) {
  if (!h || !cur || !p || !out || n_neighbours < 0 || (n_neighbours > 0 && !nbs)) return fail(DVM_ERR_INVALID, "missing argument");
  if (!cur_model || (n_neighbours > 0 && !nb_models)) return fail(DVM_ERR_INVALID, "NULL camera model");
  if (!dvm_cam::model_ok(cur_model->model, cur_model->p)) return fail(DVM_ERR_INVALID, "current keyframe: unknown camera model or zero focal length");
  for (int j = 0; j < n_neighbours; j++) {
    if (!dvm_cam::model_ok(nb_models[j].model, nb_models[j].p))
      return fail(DVM_ERR_INVALID, "neighbour " + std::to_string(j) + ": unknown camera model or zero focal length");
    if (nb_models[j].model != cur_model->model)
      return fail(DVM_ERR_INVALID, "neighbour " + std::to_string(j) + ": another camera model than the current keyframe's (a mixed pair is out of scope)");
  }
  const bool kb8 = cur_model->model == dvm_cam::kKannalaBrandt8;
  if (kb8 && n_neighbours > 0 && !nb_poses) return fail(DVM_ERR_INVALID, "missing relative poses");
  // the models' p[0..3] stand for the keyframes' fx, fy, cx, cy
  dvm_np_keyframe c = *cur;
  c.fx = cur_model->p[0]; c.fy = cur_model->p[1]; c.cx = cur_model->p[2]; c.cy = cur_model->p[3];
  std::vector<dvm_np_neighbour> nv(nbs, nbs + n_neighbours);
  for (int j = 0; j < n_neighbours; j++) {
    nv[j].kf.fx = nb_models[j].p[0]; nv[j].kf.fy = nb_models[j].p[1]; nv[j].kf.cx = nb_models[j].p[2]; nv[j].kf.cy = nb_models[j].p[3];
  }
  return create_new_map_points_impl(h, &c, n_neighbours, nv.data(), p, out, kb8, cur_model, nb_models, nb_poses);
}

int dvm_create_new_map_points_resident(dvm_new_points* h, const dvm_keyframe_store* store, const dvm_np_keyframe_resident* cur,
                                       const dvm_camera_model* cur_model, int n_neighbours, const dvm_np_neighbour_resident* nbs,
                                       const dvm_camera_model* nb_models, const dvm_pair_pose* nb_poses, const dvm_np_params* p, dvm_np_out* out) {
  if (!h || !store || !cur || !p || !out || n_neighbours < 0 || (n_neighbours > 0 && !nbs)) return fail(DVM_ERR_INVALID, "missing argument");
  if (kfs_device(store) != h->device) return fail(DVM_ERR_INVALID, "the store lives on another device than the handle");
  bool kb8 = false;
  if (cur_model) {                               // the rules of dvm_create_new_map_points_cam
    if (n_neighbours > 0 && !nb_models) return fail(DVM_ERR_INVALID, "NULL camera model");
    if (!dvm_cam::model_ok(cur_model->model, cur_model->p)) return fail(DVM_ERR_INVALID, "current keyframe: unknown camera model or zero focal length");
    for (int j = 0; j < n_neighbours; j++) {
      if (!dvm_cam::model_ok(nb_models[j].model, nb_models[j].p))
        return fail(DVM_ERR_INVALID, "neighbour " + std::to_string(j) + ": unknown camera model or zero focal length");
      if (nb_models[j].model != cur_model->model)
        return fail(DVM_ERR_INVALID, "neighbour " + std::to_string(j) + ": another camera model than the current keyframe's (a mixed pair is out of scope)");
    }
    kb8 = cur_model->model == dvm_cam::kKannalaBrandt8;
    if (kb8 && n_neighbours > 0 && !nb_poses) return fail(DVM_ERR_INVALID, "missing relative poses");
  }
  // every slot's view, then the uploaded call's structs with the slots' counts and intrinsics (or the models' p[0..3]) and the per-call part
  std::vector<KfSlotView> views((size_t)n_neighbours + 1);
  auto keyframe_of = [&](const dvm_np_keyframe_resident& r, const dvm_camera_model* m, const std::string& w, KfSlotView* v, dvm_np_keyframe* k) {
    if (!kfs_slot_view(store, r.slot, v)) return fail(DVM_ERR_INVALID, w + ": slot " + std::to_string(r.slot) + " outside the store, never written or removed");
    std::memset(k, 0, sizeof(*k));
    k->n = v->n; k->mp = r.mp; k->fv_n = v->fv_n;
    k->Tcw = r.Tcw; k->Twc = r.Twc; std::memcpy(k->Ow, r.Ow, 12);
    if (m) { k->fx = m->p[0]; k->fy = m->p[1]; k->cx = m->p[2]; k->cy = m->p[3]; }
    else { k->fx = v->fx; k->fy = v->fy; k->cx = v->cx; k->cy = v->cy; }
    k->n_levels = v->n_levels;
    return (int)DVM_OK;
  };
  dvm_np_keyframe c;
  int rc = keyframe_of(*cur, cur_model, "current keyframe", &views[0], &c);
  if (rc != DVM_OK) return rc;
  std::vector<dvm_np_neighbour> nv((size_t)n_neighbours);
  for (int j = 0; j < n_neighbours; j++) {
    rc = keyframe_of(nbs[j].kf, cur_model ? &nb_models[j] : nullptr, "neighbour " + std::to_string(j), &views[(size_t)j + 1], &nv[j].kf);
    if (rc != DVM_OK) return rc;
    nv[j].median_depth = nbs[j].median_depth;
    std::memcpy(nv[j].ep, nbs[j].ep, sizeof(nv[j].ep)); std::memcpy(nv[j].F12, nbs[j].F12, sizeof(nv[j].F12));
  }
  return create_new_map_points_impl(h, &c, n_neighbours, nv.data(), p, out, kb8, cur_model, nb_models, nb_poses, store, &views[0], views.data() + 1);
}

}  // extern "C"
