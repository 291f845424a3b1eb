// dvm_slam_amd/csrc/track_kernels.h -- launchers of track_kernels.hip (the device chain of dvm_track_finish).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h" // FrameView
#include "orb_kernels.h"   // dvm_keypoint_pod

namespace dvm {
size_t track_claims_lds(int kp_cap, int nq);
// what k_track_claims needs to search a query's window again on the device: the grid slot the ranked lists came from + the query arrays
struct TrackRequery {
  FrameView F;          // F.skp == nullptr: no device re-search (res[1] then reports the exhausted query to the caller)
  const uint8_t* qdesc; const float *qx, *qy, *qr; const int32_t *qmin, *qmax;
};
// a batch of frames through the same launches: frame b's per-query arrays at b * qstride elements (nq_arr[b] of them), its keypoints at
// b * kps_stride; count = 1, nq_arr = nullptr: one frame (nq given directly).  qoff (device, may be null): frame b's per-query arrays at
// qoff[b] elements instead (dvm_track_local_map_batch: tables of different sizes packed back to back)
struct TrackBatch {
  int count; int qstride; int64_t kps_stride; const int32_t* nq_arr; const int32_t* qoff;
  __host__ __device__ size_t qo(int b) const { return qoff ? (size_t)qoff[b] : (size_t)b * qstride; }
};
// ---- the second half (dvm_track_local_map): SearchLocalPoints -> SearchByProjection(F, points) -> PoseOptimization
struct LocalPointPod {  // == dvm_local_point
  float pos[3], normal[3], min_dist, max_dist;
  uint8_t desc[32];
  int32_t n_obs, bad;
};
// ---- the first half's queries built on the device from a map-point store (dvm_track_finish_batch_resident)
struct ResidentFrame {  // one frame of the call: its store's records, its entry count, SearchByProjection's th, the predicted pose, where its entry lists begin
  const LocalPointPod* store; int32_t n; float th; float q[4], t[3]; int32_t off;
};                      // 48 bytes
struct TrackQueryArgs { // the call's constants: camera (pinhole: fx fy cx cy; KannalaBrandt8: kb8 = mvParameters), image bounds
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y;
  float kb8[8];
};
struct TrackQueryOut {  // the tracker's device query block at the call's stride, plus what the host reads (mapped)
  uint8_t* qdesc; float *qx, *qy, *qr; int32_t *qmin, *qmax; uint8_t* q_claims; float *q_angle, *q_pos; double* pose_in; int32_t* nq_arr;
  int32_t* q_entry_host;   // mapped [count][stride]: the entry number of every query
  int32_t* nq_host;        // mapped [count]
};
// one workgroup per frame: frame b's entry lists (slot, octave, angle) at frames[b].off, its queries at b * stride, scale = mvScaleFactors [64];
// model: dvm_cam::kPinhole or kKannalaBrandt8.  The host has checked every slot against its store and every octave against the tables.
void launch_track_queries(hipStream_t s, int model, const ResidentFrame* frames, const int32_t* slot, const uint8_t* octave, const float* angle,
                          const float* scale, const TrackQueryArgs& A, int count, int stride, const TrackQueryOut& O);
struct LocalFrameArgs { int32_t n, far_points; float th, th_far; };   // one frame's table size and SearchByProjection's th / far-point filter
struct LocalMapArgs {   // the call's constants: camera, bounds, level count; per frame its table size and SearchByProjection's th / far-point filter
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y, log_scale_factor;
  int32_t n_levels;
  const LocalFrameArgs* per_frame;   // device [count]
  float kb8[8];                      // mvParameters of a KannalaBrandt8 frame (camera_model.h): read by the model-1 prologue only, which reads none of fx, fy, cx, cy
};
// what k_track_local_prologue leaves for the search (device arrays; the query arrays at the call's stride)
struct LocalQueries {
  uint8_t* qdesc; float *qx, *qy, *qr; int32_t *qmin, *qmax; uint8_t* q_claims; int32_t* q_tab;   // [stride] in table order
  int32_t* nq;                 // [1] queries
  uint8_t* seen;               // [n] the frame holds the entry
  int32_t* frame_mp;           // [kp_cap] the frame's points after the bad ones were cleared
  uint8_t* skip;               // [kp_cap] keypoint holds a point with Observations() > 0
  float* pos;                  // [n][3] GetWorldPos() of every entry (the edge gather's positions)
  uint8_t* claims;             // [n] Observations() > 0 of every entry
  double* pose_in;             // [7] the first half's float pose widened: PoseOptimization's seed
};
// pose_first: the first half's optimised poses (t, q doubles); scale: mvScaleFactors [64]; B: count frames with B.qoff (frame b's table,
// per-entry and query arrays at qoff[b], its per-keypoint arrays at b * kp_cap, A.per_frame[b]); model: dvm_cam::kPinhole or kKannalaBrandt8
// (mpCamera->project of isInFrustum through A.kb8)
void launch_track_local_prologue(hipStream_t s, int model, const LocalPointPod* pts, const int32_t* frame_mp_in, const double* pose_first, const float* scale,
                                 const int32_t* d_n, int kp_cap, const LocalMapArgs& A, const LocalQueries& LQ, TrackPoint* track_pts_host,
                                 int32_t* res_host, const TrackBatch& B);
// the claim replay of SearchByProjection(F, points) (k_track_claims<true>): assign[j] = the table entry keypoint j holds at the end (the
// matched query's entry, else frame_mp[j]); res[0] = nmatches, res[3] = queries searched again
void launch_track_claims_local(hipStream_t s, const uint32_t* ranked, const LocalQueries& LQ, const TrackRequery& rq, const dvm_keypoint_pod* kps,
                               const int32_t* d_n, int kp_cap, int th_high, float nnratio, int32_t* assign, int32_t* res, int32_t* assign_host,
                               int32_t* res_host, const TrackBatch& B);
void launch_track_claims(hipStream_t s, const uint32_t* ranked, const uint8_t* q_claims, const float* q_angle, int nq, const TrackRequery& rq,
                         const dvm_keypoint_pod* kps, const int32_t* d_n, int kp_cap, int th_high, int check_ori, int32_t* assign, int32_t* res,
                         int32_t* assign_host, int32_t* res_host, const TrackBatch& B);
void launch_track_gather(hipStream_t s, const int32_t* assign, const dvm_keypoint_pod* kps_un, const int32_t* d_n, int kp_cap, const float* q_pos,
                         const float* inv_sigma2, int nlevels, double* Xw, double* obs, double* info, int32_t* edge_kp, int32_t* n_edges,
                         const int32_t* res, int min_matches, int32_t* n_edges_host, const TrackBatch& B);
void launch_track_finish(hipStream_t s, int32_t* assign, const int32_t* d_n, int kp_cap, const int32_t* edge_kp, const int32_t* n_edges,
                         const uint8_t* edge_outlier, const uint8_t* q_claims, uint8_t* outlier, int32_t* out, const int32_t* res, const TrackBatch& B);

// ---- the reference-keyframe chain (dvm_track_reference_keyframe): Frame::ComputeBoW -> SearchByBoW(KF, F) -> PoseOptimization
constexpr int kRefKfCnt = 40;   // RefKfArgs::cnt entries: [0] n_bow [1] n_fv [2] matches before the rotation check [8, 38) rotation histogram
struct RefKfArgs {
  // the frame: k_vocab_transform's per-feature word / node / weight [cap]
  const int32_t* word; const int32_t* node; const double* w;
  int32_t *fv_node, *fv_off, *fv_feat;   // device: mFeatVec as CSR ([cap], [cap + 1], [cap])
  int32_t* cnt;                          // device [kRefKfCnt]
  int32_t* match;                        // device [cap]: the keyframe keypoint matched to frame keypoint j, or -1 (k_track_gather's assign)
  int32_t* bin;                          // device [cap]: its rotation bin
  int32_t* res;                          // device [8]: res[0] = nmatches, res[1] = 0 (what k_track_gather / k_track_finish read)
  // mapped host memory: what the host reads after the one synchronisation
  int32_t* h_bow_ids; double* h_bow_vals; int32_t *h_fv_node, *h_fv_off, *h_fv_feat; int32_t* h_match; int32_t* h_cnt;
  // the keyframe (device copy of the upload)
  const uint8_t* kdesc; const float* kangle; const uint8_t* kuse;   // [n]: descriptor, mvKeysUn angle, has a good map point
  const int32_t *kfv_node, *kfv_off, *kfv_feat;                     // its mFeatVec
  // the frames (one frame is a batch of one): frame b's per-frame arrays above at b * cap (fv_off at b * (cap + 1), cnt at b * kRefKfCnt,
  // res at 8 b, h_cnt at 8 b), its keyframe at kqoff[b] entries of the upload (kfv_off at kqoff[b] + b), its frame inputs at
  // b * kps_stride / b * desc_stride
  const int32_t* run;       // device [nrun]: the frames that run; workgroup r of the bow / settle kernels works on frame run[r]
  const int32_t* kqoff;     // device [count]
  const int32_t* kfv_nb;    // device [count]: the keyframes' node counts
  const int32_t* wg_base;   // device [nrun + 1]: run r's first workgroup of k_refkf_search (its nodes, 4 per workgroup)
  int32_t nrun, nwg;        // frames that run, k_refkf_search's workgroups (host values)
  int64_t kps_stride, desc_stride;
};
// one workgroup (per frame that runs): the frame's BowVector (mapped) and FeatureVector (device + mapped); the match state reset
void launch_refkf_bow(hipStream_t s, const RefKfArgs& A, const int32_t* d_n, int cap);
// SearchByBoW's matching: one wave per keyframe node (each frame its own range of workgroups, A.wg_base); then the rotation check and
// res[] for the edge gather, one workgroup per frame that runs
void launch_refkf_search(hipStream_t s, const RefKfArgs& A, const dvm_keypoint_pod* kps_un, const uint8_t* desc, const int32_t* d_n, int cap, int th_low,
                         float nnratio);
void launch_refkf_settle(hipStream_t s, const RefKfArgs& A, const int32_t* d_n, int cap, int check_ori);
// ---- the packed keyframes of the chain above filled on the device (dvm_track_reference_keyframe_batch_resident): frame b's keyframe is a
// keyframe-store slot (kps, desc, the FeatureVector) plus its map points as slots of a map store (recs)
struct RefKfGatherItem {
  const LocalPointPod* recs;              // the frame's map store; not read when every mp_slot < 0
  const dvm_keypoint_pod* kps; const uint8_t* desc; const int32_t *fv_node, *fv_off, *fv_feat;   // in the slot
  int32_t n, n_feat;                      // keypoints, features the FeatureVector lists (its node count: kfv_nb[b])
};                                        // 56 bytes
struct RefKfGatherOut { uint8_t* desc; float* angle; uint8_t *use, *claims; float* pos; int32_t *fv_node, *fv_feat, *fv_off; };
// one workgroup per frame that runs (run [nrun]): frame b's keyframe written at kqoff[b] entries of O (fv_off at kqoff[b] + b) as the
// uploaded call packs it; mp_slot: the frames' lists at kqoff[b].  The host has checked every slot of every list.
void launch_refkf_gather(hipStream_t s, const RefKfGatherItem* items, const int32_t* mp_slot, const int32_t* run, int nrun, const int32_t* kqoff,
                         const int32_t* kfv_nb, const RefKfGatherOut& O);
}  // namespace dvm
