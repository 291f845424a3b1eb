// dvm_slam_amd/csrc/track_layout.h -- the byte layouts of dvm_tracker's working sets (track.cpp), each written ONCE: a carve_* function
// walks a block with a Cursor (chain.h) and returns the items' pointers and the bytes used.  A reservation calls it on a null base at the
// largest arguments for the size; a call carves the same function on the real block at its own count / stride / table size, which fits
// because every item only grows with those (tools/check_track_layout.cpp walks the grid).  Host-only: no kernel reads a struct of this file.
#pragma once
#include "chain.h"
#include "match_kernels.h"   // TrackPoint
#include "track_kernels.h"

namespace dvm {

// ---- the first half (dvm_tracker_create_batch): B = max_frames, K = max_keypoints, Q = max_queries rounded up to 64
// device, [frame][...]; q: the query block's device copy (qbytes), the block's last item
struct TrackerDevice {
  uint32_t* ranked; int32_t *assign, *res; double *Xw, *obs, *info, *chi; int32_t *edge_kp, *nedges; uint8_t* edge_out; dvm_keypoint_pod* kps_un;
  uint8_t* q; size_t bytes;
};
inline TrackerDevice carve_tracker_device(uint8_t* base, size_t B, size_t K, size_t Q, size_t qbytes) {
  TrackerDevice d;
  Cursor<256> c{base};
  d.ranked = c.carve<uint32_t>(B * Q * 4); d.assign = c.carve<int32_t>(B * K); d.res = c.carve<int32_t>(B * 8);
  d.Xw = c.carve<double>(B * K * 3); d.obs = c.carve<double>(B * K * 2); d.info = c.carve<double>(B * K); d.chi = c.carve<double>(B * K);
  d.edge_kp = c.carve<int32_t>(B * K); d.nedges = c.carve<int32_t>(B); d.edge_out = c.carve<uint8_t>(B * K);
  d.kps_un = c.carve<dvm_keypoint_pod>(B * K); d.q = c.carve<uint8_t>(qbytes);
  d.bytes = c.used();
  return d;
}
// the query block of a call of `count` frames at stride Qs (a multiple of 64), at the head of the mapped buffer and of its device copy
struct QueryBlock {
  uint8_t* qdesc; float *qx, *qy, *qr; int32_t *qmin, *qmax; uint8_t* q_claims; float *q_angle, *q_pos; double* pose_in; int32_t* nq_arr;
  float* inv_sigma2; size_t bytes;
};
inline QueryBlock carve_query_block(uint8_t* base, size_t count, size_t Qs) {
  QueryBlock m;
  Cursor<256> c{base};
  const size_t Qn = count * Qs;
  m.qdesc = c.carve<uint8_t>(Qn * 32); m.qx = c.carve<float>(Qn); m.qy = c.carve<float>(Qn); m.qr = c.carve<float>(Qn);
  m.qmin = c.carve<int32_t>(Qn); m.qmax = c.carve<int32_t>(Qn); m.q_claims = c.carve<uint8_t>(Qn); m.q_angle = c.carve<float>(Qn);
  m.q_pos = c.carve<float>(Qn * 3); m.pose_in = c.carve<double>(count * 7); m.nq_arr = c.carve<int32_t>(count); m.inv_sigma2 = c.carve<float>(64);
  m.bytes = c.used();
  return m;
}
// the mapped results behind the query block (host address; device address: ws.dev(p)); kps_un: one frame's (the single call's undistortion)
struct TrackerResults {
  int32_t* assign; uint8_t* outlier; int32_t *res, *fin, *nedges; double* pose_out; int32_t* n_inl; dvm_keypoint_pod* kps_un; size_t bytes;
};
inline TrackerResults carve_tracker_results(uint8_t* base, size_t B, size_t K) {
  TrackerResults m;
  Cursor<256> c{base};
  m.assign = c.carve<int32_t>(B * K); m.outlier = c.carve<uint8_t>(B * K);
  m.res = c.carve<int32_t>(B * 8); m.fin = c.carve<int32_t>(B * 4); m.nedges = c.carve<int32_t>(B); m.pose_out = c.carve<double>(B * 7);
  m.n_inl = c.carve<int32_t>(B); m.kps_un = c.carve<dvm_keypoint_pod>(K);
  m.bytes = c.used();
  return m;
}

// ---- the resident first half.  The upload block, carved in the mapped staging buffer and at the same offsets in its device copy:
// [mvScaleFactors 64][mvInvLevelSigma2 64][frames][slot, angle, octave: E entries each, frame b's at ResidentFrame::off -- every frame's
// list rounded up to 64 entries, back to back] -- 9 bytes per entry
struct ResidentUpload { float *scale, *inv_sigma2; ResidentFrame* fr; int32_t* slot; float* angle; uint8_t* octave; size_t bytes; };
inline ResidentUpload carve_resident_upload(uint8_t* base, size_t count, size_t E) {
  ResidentUpload u;
  Cursor<64> c{base};
  u.scale = c.carve<float>(64); u.inv_sigma2 = c.carve<float>(64); u.fr = c.carve<ResidentFrame>(count);
  u.slot = c.carve<int32_t>(E); u.angle = c.carve<float>(E); u.octave = c.carve<uint8_t>(E);
  u.bytes = c.used();
  return u;
}
// the mapped buffer of the resident first half: [the upload's staging: up bytes][q_entry: B x Q][nq: B]; up: the largest upload, rounded
struct ResidentMapped { int32_t *entry, *nq; size_t up, bytes; };
inline ResidentMapped carve_resident_mapped(uint8_t* base, size_t B, size_t Q) {
  ResidentMapped r;
  Cursor<256> c{base};
  c.carve<uint8_t>(carve_resident_upload(nullptr, B, B * Q).bytes);
  r.up = c.used();
  r.entry = c.carve<int32_t>(B * Q); r.nq = c.carve<int32_t>(B);
  r.bytes = c.used();
  return r;
}

// ---- the second half (dvm_tracker_reserve_local_map): P = table entries of one call (a multiple of 64).  The upload block of one call,
// carved in the mapped staging buffer and at the same offsets in the device copy: [mvScaleFactors 64][mvInvLevelSigma2 64][per frame: the
// first half's pose 7 doubles, LocalFrameArgs, table offset, skip-flag switch][tables: T records, frame b's at qoff[b]][frame_mp: count x kstride]
struct LocalMapUpload {
  float *scale, *inv_sigma2; double* pose; LocalFrameArgs* fa; int32_t *qoff, *skip_on; LocalPointPod* pts; int32_t* frame_mp; size_t bytes;
};
// the head both forms begin with: the level tables and the frame block (one item; its four arrays back to back)
inline void carve_local_map_head(Cursor<256>& c, size_t count, LocalMapUpload& u) {
  u.scale = c.carve<float>(64); u.inv_sigma2 = c.carve<float>(64);
  Cursor<4> f{c.carve<uint8_t>(count * (7 * 8 + sizeof(LocalFrameArgs) + 8))};
  u.pose = f.carve<double>(count * 7); u.fa = f.carve<LocalFrameArgs>(count); u.qoff = f.carve<int32_t>(count); u.skip_on = f.carve<int32_t>(count);
}
inline LocalMapUpload carve_local_map_upload(uint8_t* base, size_t count, size_t T, size_t kstride) {
  LocalMapUpload u;
  Cursor<256> c{base};
  carve_local_map_head(c, count, u);
  u.pts = c.carve<LocalPointPod>(T); u.frame_mp = c.carve<int32_t>(count * kstride);
  u.bytes = c.used();
  return u;
}
// the same block where the tables are store slots (dvm_track_local_map_batch_resident): [head][the frames' stores: count device pointers]
// [slots: T, frame b's at qoff[b]][frame_mp: count x kstride] -- copied up to here (copy_bytes) in one copy -- then [tables: T records],
// device only: k_store_gather fills them from the stores
struct LocalMapUploadResident { LocalMapUpload u; const LocalPointPod** stores; int32_t* slots; size_t copy_bytes; };
inline LocalMapUploadResident carve_local_map_upload_resident(uint8_t* base, size_t count, size_t T, size_t kstride) {
  LocalMapUploadResident r;
  LocalMapUpload& u = r.u;
  Cursor<256> c{base};
  carve_local_map_head(c, count, u);
  Cursor<64> t{base, nullptr, c.used()};
  r.stores = t.carve<const LocalPointPod*>(count); r.slots = t.carve<int32_t>(T);
  r.copy_bytes = t.used() + count * kstride * 4;
  u.frame_mp = t.carve<int32_t>(count * kstride);
  c.off = pad<256>(r.copy_bytes);
  u.pts = c.carve<LocalPointPod>(T);
  u.bytes = c.used();
  return r;
}
// the upload region reserved for either form: the record form's block with the resident form's slot list and store pointers behind it as
// items of their own.  (More than either form uses -- the resident carve packs those two in 64-byte items before frame_mp -- and kept.)
inline size_t local_map_upload_capacity(size_t B, size_t P, size_t K) {
  Cursor<256> c{nullptr, nullptr, carve_local_map_upload(nullptr, B, P, K).bytes};
  c.carve<int32_t>(P); c.carve<const LocalPointPod*>(B);
  return c.used();
}
// the device arrays of one call behind the upload region: per entry at the frames' offsets (T entries), per keypoint at b * ocap
struct LocalMapWork { LocalQueries LQ; uint32_t* ranked; int32_t* lres; size_t bytes; };
inline LocalMapWork carve_local_map_work(uint8_t* base, size_t count, size_t T, size_t ocap) {
  LocalMapWork w;
  LocalQueries& LQ = w.LQ;
  Cursor<256> c{base};
  const size_t Kb = count * ocap;
  LQ.seen = c.carve<uint8_t>(T); LQ.pos = c.carve<float>(T * 3); LQ.claims = c.carve<uint8_t>(T);
  LQ.frame_mp = c.carve<int32_t>(Kb); LQ.skip = c.carve<uint8_t>(Kb); LQ.pose_in = c.carve<double>(count * 7);
  LQ.qdesc = c.carve<uint8_t>(T * 32); LQ.qx = c.carve<float>(T); LQ.qy = c.carve<float>(T); LQ.qr = c.carve<float>(T);
  LQ.qmin = c.carve<int32_t>(T); LQ.qmax = c.carve<int32_t>(T); LQ.q_claims = c.carve<uint8_t>(T); LQ.q_tab = c.carve<int32_t>(T);
  w.ranked = c.carve<uint32_t>(T * 4);
  w.lres = c.carve<int32_t>(count * 8);
  LQ.nq = c.carve<int32_t>(count * 8);
  w.bytes = c.used();
  return w;
}
// the mapped results behind the upload staging, [max_frames] slices (tp: the call's table entries)
struct LocalMapResults { int32_t* mp; uint8_t* outlier; TrackPoint* tp; int32_t* res; double* pose; int32_t *n_inl, *fin, *nedges; size_t bytes; };
inline LocalMapResults carve_local_map_results(uint8_t* base, size_t B, size_t K, size_t P) {
  LocalMapResults r;
  Cursor<256> c{base};
  r.mp = c.carve<int32_t>(B * K); r.outlier = c.carve<uint8_t>(B * K); r.tp = c.carve<TrackPoint>(P); r.res = c.carve<int32_t>(B * 16);
  r.pose = c.carve<double>(B * 7); r.n_inl = c.carve<int32_t>(B * 4); r.fin = c.carve<int32_t>(B * 4); r.nedges = c.carve<int32_t>(B * 4);
  r.bytes = c.used();
  return r;
}

// ---- TrackReferenceKeyFrame.  The upload block of one call: [mvInvLevelSigma2 64][per frame: pose_in 7 doubles, keyframe offset, node
// count, res 8][run list][wg_base][keyframes: T entries, frame b's at qoff[b] -- desc x 32, angle, use, claims, pos x 3, mFeatVec nodes,
// features][mFeatVec offsets: T + count, frame b's at qoff[b] + b]
struct KeyframeUpload {
  float* inv_sigma2; double* pose; int32_t *qoff, *kfv_n, *res, *run, *wg_base;
  uint8_t* desc; float* angle; uint8_t *use, *claims; float* pos; int32_t *fv_node, *fv_feat, *fv_off; size_t bytes;
};
// the head both forms begin with, and the packed keyframes the chain's kernels read at kqoff[b]
inline void carve_keyframe_head(Cursor<256>& c, size_t B, KeyframeUpload& u) {
  u.inv_sigma2 = c.carve<float>(64); u.pose = c.carve<double>(B * 7); u.qoff = c.carve<int32_t>(B); u.kfv_n = c.carve<int32_t>(B);
  u.res = c.carve<int32_t>(B * 8); u.run = c.carve<int32_t>(B); u.wg_base = c.carve<int32_t>(B + 1);
}
inline void carve_keyframe_block(Cursor<256>& c, size_t B, size_t T, KeyframeUpload& u) {
  u.desc = c.carve<uint8_t>(T * 32); u.angle = c.carve<float>(T); u.use = c.carve<uint8_t>(T); u.claims = c.carve<uint8_t>(T);
  u.pos = c.carve<float>(T * 3); u.fv_node = c.carve<int32_t>(T); u.fv_feat = c.carve<int32_t>(T); u.fv_off = c.carve<int32_t>(T + B);
}
inline KeyframeUpload carve_keyframe_upload(uint8_t* base, size_t B, size_t T) {
  KeyframeUpload u;
  Cursor<256> c{base};
  carve_keyframe_head(c, B, u); carve_keyframe_block(c, B, T, u);
  u.bytes = c.used();
  return u;
}
// the same block where the keyframes are store slots (dvm_track_reference_keyframe_batch_resident): [head][per frame: where k_refkf_gather
// reads the keyframe][mp_slot: T entries, frame b's at qoff[b]] -- copied up to here (copy_bytes) in one copy -- then [keyframes: T
// entries][offsets], device only: k_refkf_gather fills them from the slots and the map stores
struct KeyframeUploadResident { KeyframeUpload u; RefKfGatherItem* items; int32_t* mp_slot; size_t copy_bytes; };
inline KeyframeUploadResident carve_keyframe_upload_resident(uint8_t* base, size_t B, size_t T) {
  KeyframeUploadResident r;
  Cursor<256> c{base};
  carve_keyframe_head(c, B, r.u);
  r.items = c.carve<RefKfGatherItem>(B); r.mp_slot = c.carve<int32_t>(T);
  r.copy_bytes = c.used();
  carve_keyframe_block(c, B, T, r.u);
  r.u.bytes = c.used();
  return r;
}
// the device working set behind the upload, per frame at the call's capacity stride (cap <= kp_cap, count <= max_frames)
struct RefKfWork { int32_t *word, *node; double* w; int32_t *fv_node, *fv_feat, *fv_off, *cnt, *match, *bin; size_t bytes; };
inline RefKfWork carve_refkf_work(uint8_t* base, size_t B, size_t K) {
  RefKfWork r;
  Cursor<256> c{base};
  r.word = c.carve<int32_t>(B * K); r.node = c.carve<int32_t>(B * K); r.w = c.carve<double>(B * K);
  r.fv_node = c.carve<int32_t>(B * K); r.fv_feat = c.carve<int32_t>(B * K); r.fv_off = c.carve<int32_t>(B * (K + 1));
  r.cnt = c.carve<int32_t>(B * kRefKfCnt); r.match = c.carve<int32_t>(B * K); r.bin = c.carve<int32_t>(B * K);
  r.bytes = c.used();
  return r;
}
// the mapped results behind the upload staging: BowVector, FeatureVector, match, counters, outlier flags, edges / inliers / nmatchesMap,
// pose, B slices each (fv_off: K + 1 per frame, cnt: 8 per frame)
struct RefKfMapped {
  int32_t *bow_ids, *fv_node, *fv_off, *fv_feat, *match, *cnt, *nedges, *n_inl, *fin; double *bow_vals, *pose; uint8_t* outlier; size_t bytes;
};
inline RefKfMapped carve_refkf_results(uint8_t* base, size_t B, size_t K) {
  RefKfMapped r;
  Cursor<256> c{base};
  r.bow_ids = c.carve<int32_t>(B * K); r.bow_vals = c.carve<double>(B * K); r.fv_node = c.carve<int32_t>(B * K); r.fv_feat = c.carve<int32_t>(B * K);
  r.fv_off = c.carve<int32_t>(B * (K + 1)); r.match = c.carve<int32_t>(B * K); r.cnt = c.carve<int32_t>(B * 8); r.outlier = c.carve<uint8_t>(B * K);
  r.nedges = c.carve<int32_t>(B * 4); r.n_inl = c.carve<int32_t>(B * 4); r.fin = c.carve<int32_t>(B * 4); r.pose = c.carve<double>(B * 7);
  r.bytes = c.used();
  return r;
}

}  // namespace dvm
