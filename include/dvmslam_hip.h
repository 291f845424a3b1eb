/*
 * include/dvmslam_hip.h -- C ABI of libdvmslam_hip.so: the MI355X (gfx950) implementation of the
 * per-agent visual-SLAM hot path of proroklab/DVM-SLAM (ORB front end, Hamming matching, bundle
 * adjustment).  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Reference interface replaced (all under /root/reference/src/slam_system/orb_slam3/):
 *   dvm_orb_*      <- class ORBextractor            include/ORBextractor.h:47-91, src/ORBextractor.cc:282-976
 *   dvm_frame_*    <- Frame grid members            include/Frame.h:44-45,221-251, src/Frame.cc:443-506,712-782
 *   dvm_hamming_*  <- ORBmatcher::DescriptorDistance include/ORBmatcher.h:44, src/ORBmatcher.cc:1900-1914
 *   dvm_match_*    <- inner loops of ORBmatcher::SearchByProjection / SearchForInitialization
 *                                                    src/ORBmatcher.cc:44-205,605-707,1553-1748
 *   dvm_ba_*       <- Optimizer::{BundleAdjustment,LocalBundleAdjustment} + g2o BlockSolver_6_3/LM
 *                                                    src/Optimizer.cc:55-356,1030-1387
 *   dvm_pose_optimize <- Optimizer::PoseOptimization src/Optimizer.cc:744-1028
 *   dvm_pose_optimize_cam, dvm_is_in_frustum_cam, dvm_project_search_cam <- the same on a GeometricCamera (CameraModels/KannalaBrandt8.cpp)
 *   dvm_match_triangulation_cam, dvm_triangulate_matches_cam, dvm_create_new_map_points_cam <- CreateNewMapPoints on such a camera
 *   dvm_pose_graph_optimize <- Optimizer::OptimizeEssentialGraph src/Optimizer.cc:1389-1652 (g2o part)
 *   dvm_sim3_hypotheses <- Sim3Solver::ComputeSim3 + CheckInliers src/Sim3Solver.cc:294-408
 *   dvm_distinctive_descriptors <- MapPoint::ComputeDistinctiveDescriptors src/MapPoint.cc:384-453
 *   dvm_vocab_transform <- DBoW2::TemplatedVocabulary::transform Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1098-1138
 * The reference has no FFI: these classes live inside static libORB_SLAM3.a.  INTEGRATION.md shows
 * the C++ shim classes (same names / signatures) a maintainer links instead.
 *
 * Conventions: every function returns DVM_OK (0) or a negative dvm_status; nothing throws across
 * the boundary.  A handle owns one HIP stream and all of its device memory; handles are not
 * thread-safe (one per calling thread, like the reference's ORBextractor instance per Tracking).
 * Pointers named d_* are DEVICE pointers (HBM), all others are host pointers.
 */
#ifndef DVMSLAM_HIP_H
#define DVMSLAM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DVM_OK = 0,
  DVM_ERR_INVALID = -1,    /* bad argument */
  DVM_ERR_EMPTY = -2,      /* empty image: the reference's operator() returns -1 (ORBextractor.cc:879-880) */
  DVM_ERR_CAPACITY = -3,   /* caller buffer too small */
  DVM_ERR_HIP = -4,        /* HIP runtime error (see dvm_last_error) */
  DVM_ERR_NO_DEVICE = -5,  /* no gfx950 device visible: the library never falls back to a CPU path */
  DVM_ERR_STATE = -6       /* call sequence error */
} dvm_status;

const char* dvm_last_error(void);
const char* dvm_version(void);
/* number of visible HIP devices (0 when none); never fails */
int dvm_device_count(void);
/* makes `device` the calling THREAD's current HIP device.  Entry points that take a handle or a device argument select their GPU
 * themselves; the stateless ones without either (dvm_hamming_matrix, dvm_is_in_frustum, dvm_triangulate_matches,
 * dvm_undistort_keypoints, dvm_match_lists, dvm_match_triangulation, dvm_distinctive_descriptors, dvm_pose_optimize's host form ...)
 * run on the calling thread's current device -- 0 on a fresh thread.  An agent pinned to GPU k calls this once per thread (the shims
 * of dvm_slam_amd/host do it through dvm_host::use_device()).  DVM_ERR_NO_DEVICE / DVM_ERR_INVALID as for the handle constructors. */
int dvm_set_device(int device);

/* layout-identical to cv::KeyPoint (7 x 4 B): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} dvm_keypoint;

/* ------------------------------------------------------------------------------ ORB extractor */
/* ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST) */
typedef struct {
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels, ini_th_fast, min_th_fast;
} dvm_orb_params;

typedef struct dvm_orb dvm_orb;

/* max_batch: frames processed per launch set (>=1).  Device buffers are sized lazily for the first
 * image size seen and re-sized when it changes. */
int dvm_orb_create(const dvm_orb_params* p, int device, int max_batch, dvm_orb** out);
void dvm_orb_destroy(dvm_orb* h);
/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares and
 * mnFeaturesPerLevel; arrays of nlevels entries, any may be NULL */
int dvm_orb_tables(const dvm_orb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                   int32_t* nfeat_per_level);

/* operator()(image, mask, keypoints, descriptors, vLappingArea): one host image in, host results
 * out (synchronous).  *n = number of keypoints, *mono_index = the reference's return value.
 * desc receives n x 32 bytes.  Returns DVM_ERR_EMPTY for a null / zero-sized image. */
int dvm_orb_extract(dvm_orb* h, const uint8_t* img, int rows, int cols, int stride, int lap0, int lap1,
                    dvm_keypoint* kps, uint8_t* desc, int cap, int* n, int* mono_index);

/* A SHARED extractor for several agents' frames.  The reference runs one ORBextractor per agent, each called once per frame from that
 * agent's tracking thread (Tracking.cc:1423-1426; orb_slam3_wrapper.cpp runs one System per agent).  K such threads on one GPU issue K
 * chains of small launches that serialise in the runtime; dvm_orb_pool_extract is the same blocking call -- one image in, that
 * frame's keypoints and descriptors out, the same bytes as dvm_orb_extract -- but frames that arrive within `window_us` of each other
 * (and share size and lapping area) are extracted as ONE batch of up to max_batch frames: the caller that opened the batch waits for
 * the arrivals to pause, runs it, and every caller copies its own frame's results out.  Four batches are in flight (one collecting while
 * others run; max_batch 8 measured best: small overlapping batches beat large ones that keep the agents in lockstep).  Callable from any number of threads at once; window_us < 0: 20 us; a caller that has been alone for eight calls stops waiting.
 * batch_size (may be NULL): how many frames the call's batch held.  Destroy a pool only when no call on it is in flight (this holds for
 * dvm_pose_pool and dvm_match_pool too). */
typedef struct dvm_orb_pool dvm_orb_pool;
int dvm_orb_pool_create(const dvm_orb_params* p, int device, int max_batch, int window_us, dvm_orb_pool** out);
void dvm_orb_pool_destroy(dvm_orb_pool* pool);
int dvm_orb_pool_extract(dvm_orb_pool* pool, const uint8_t* img, int rows, int cols, int stride, int lap0, int lap1, dvm_keypoint* kps,
                         uint8_t* desc, int cap, int* n, int* mono_index, int* batch_size);

/* Batched, device-resident form: `batch` frames of rows x cols at d_imgs + f*frame_stride (bytes),
 * row pitch `stride`.  Asynchronous on the handle's stream; results stay in HBM until fetched. */
int dvm_orb_extract_batch_device(dvm_orb* h, const uint8_t* d_imgs, int batch, int rows, int cols, int stride,
                                 int64_t frame_stride, int lap0, int lap1);
/* Same, from host memory (one pinned staging copy + H2D on the handle's stream). */
int dvm_orb_extract_batch_host(dvm_orb* h, const uint8_t* imgs, int batch, int rows, int cols, int stride,
                               int64_t frame_stride, int lap0, int lap1);
/* blocks until the handle's stream is idle */
/* Pinned-staging ingest: dvm_orb_staging returns the handle's page-locked input buffer (batch x rows x cols bytes, rows
 * tight) for the caller -- camera driver, decoder -- to write frames into; dvm_orb_extract_staged queues the PCIe copy and
 * the extraction on the handle's stream and returns without waiting.  dvm_orb_staging waits for the previous copy out of
 * the buffer.  Two handles used alternately overlap one batch's transfer with the other's kernels. */
int dvm_orb_staging(dvm_orb* h, int batch, int rows, int cols, uint8_t** host_ptr);
int dvm_orb_extract_staged(dvm_orb* h, int batch, int rows, int cols, int lap0, int lap1);
int dvm_orb_sync(dvm_orb* h);
/* device views of frame f's results (valid until the next extract on this handle).  kps are in
 * the reference's output order; d_n points at the int32 keypoint count of the frame. */
int dvm_orb_result_device(dvm_orb* h, int frame, const dvm_keypoint** d_kps, const uint8_t** d_desc,
                          const int32_t** d_n, int* capacity);
/* A reference to the keypoints + descriptors a single-frame dvm_orb_extract has just produced, still in HBM: a plain value the
 * caller keeps beside the host copies (the Frame that owns mvKeys / mDescriptors -- Frame.cc:411 -- and every copy of that Frame) and
 * hands to the consumers of the same data (dvm_frame_build through dvmh_frame_view::dev: the grid of SearchByProjection is then
 * built from the device arrays, no second upload).  The arrays live until the handle extracts again or is destroyed;
 * dvm_device_frame_valid tells (0 / 1) whether a reference still names the handle's current result. */
typedef struct {
  const dvm_keypoint* d_kps;
  const uint8_t* d_desc;
  int32_t n, device;
  uint64_t handle_id, serial;
} dvm_device_frame;
int dvm_orb_last_result(dvm_orb* h, dvm_device_frame* out);
int dvm_device_frame_valid(const dvm_device_frame* ref);
/* asynchronous device-to-device copy (on the handle's stream) of frame f's keypoints, descriptors
 * and count into caller-owned device buffers (capacity as reported by dvm_orb_result_device) --
 * used to carry the last frame of a batch over to the next batch's frame-to-frame search */
int dvm_orb_copy_result(dvm_orb* h, int frame, dvm_keypoint* d_kps_dst, uint8_t* d_desc_dst, int32_t* d_n_dst);
/* device array of mvScaleFactor (nlevels floats) */
const float* dvm_orb_scale_factors_device(dvm_orb* h);
/* synchronises, then copies frame f's results to the host */
int dvm_orb_download(dvm_orb* h, int frame, dvm_keypoint* kps, uint8_t* desc, int cap, int* n, int* mono_index);
/* the first `count` frames of the last batch in one go (one synchronisation, two block copies through page-locked memory): kps[f] / desc[f]
 * with caps[f] entries, n[f], mono_index[f] */
int dvm_orb_download_batch(dvm_orb* h, int count, dvm_keypoint* const* kps, uint8_t* const* desc, const int* caps, int* n, int* mono_index);
/* mvImagePyramid[level] of frame f: device pointer to pixel (0,0) of the level; the 19-px
 * REFLECT_101 border is addressable at negative offsets exactly like the reference's ROI Mats */
int dvm_orb_pyramid(dvm_orb* h, int frame, int level, const uint8_t** d_ptr, int* rows, int* cols, int* stride);

/* stage-wise intermediates of frame f (parity tests; each synchronises) */
int dvm_orb_debug_level(dvm_orb* h, int frame, int level, int bordered, uint8_t* out /* tight rows */);
int dvm_orb_debug_blurred(dvm_orb* h, int frame, int level, uint8_t* out);
int dvm_orb_debug_candidates(dvm_orb* h, int frame, int level, int32_t* xs, int32_t* ys, int32_t* scores,
                             int cap, int* n);
int dvm_orb_debug_level_keypoints(dvm_orb* h, int frame, int level, dvm_keypoint* kps, int cap, int* n);
/* *out = 1 if the last batch built pyramid level `level` with k_pyr_resize_direct, 0 for k_pyr_resize (and for level 0) */
int dvm_orb_debug_pyr_path(dvm_orb* h, int level, int* out);

/* per-kernel HIP-event timing on the handle's stream.  names: "pyramid","fast","octree",
 * "assemble","blur","orient_desc","grid_sort","match" ...  Returns accumulated milliseconds and launch count since
 * the last reset. */
int dvm_orb_profiling(dvm_orb* h, int enable);
int dvm_orb_profile_get(dvm_orb* h, const char* name, double* total_ms, int64_t* launches);
int dvm_orb_profile_reset(dvm_orb* h);
/* the handle's hipStream_t (so callers can order their own work / events against it) */
void* dvm_orb_stream(dvm_orb* h);

/* ----------------------------------------------------------------------------------- matching */
/* DescriptorDistance for all pairs: D[i*nB+j] = popcount(A[i]^B[j]) over 256 bits (uint16).
 * on_device != 0: A, B, D are device pointers and the call is asynchronous on `stream`
 * (hipStream_t, may be NULL for the default stream); otherwise host pointers, synchronous. */
int dvm_hamming_matrix(const uint8_t* A, int nA, const uint8_t* B, int nB, uint16_t* D, int on_device, void* stream);

/* Frame feature grid (FRAME_GRID_COLS=64 x FRAME_GRID_ROWS=48) + windowed best/second-best search.
 * A dvm_frame holds `slots` frames' undistorted keypoints + descriptors in HBM, each ordered the
 * way Frame::GetFeaturesInArea enumerates them, so ties resolve exactly like the reference's loops.
 * capacity <= 8192 keypoints per slot. */
typedef struct dvm_frame dvm_frame;
int dvm_frame_create(int device, int capacity, int slots, dvm_frame** out);
void dvm_frame_destroy(dvm_frame* f);
/* (Re)build slot `slot` from n keypoints + descriptors; on_device selects pointer kind; d_n (device
 * int32*, may be NULL, only with on_device) overrides n with a device-side count.  Bounds are
 * Frame::mnMinX/mnMaxX/mnMinY/mnMaxY (0,cols,0,rows when undistorted) and apply to all slots.
 * Asynchronous on `stream` when on_device (host pointers: synchronous). */
int dvm_frame_build(dvm_frame* f, int slot, const dvm_keypoint* kps, const uint8_t* desc, int n, const int32_t* d_n,
                    float minX, float maxX, float minY, float maxY, int on_device, void* stream);
/* Build slots [first_slot, first_slot+count) from device arrays d_kps + i*kps_stride (elements),
 * d_desc + i*desc_stride (bytes), counts d_n[i] -- the layout dvm_orb_result_device exposes. */
int dvm_frame_build_batch(dvm_frame* f, int first_slot, int count, const dvm_keypoint* d_kps, int64_t kps_stride,
                          const uint8_t* d_desc, int64_t desc_stride, const int32_t* d_n, float minX, float maxX,
                          float minY, float maxY, void* stream);
/* Device-side counts (d_n of dvm_frame_build[_batch], the per-frame counts of dvm_match_frames_batch) larger than the handle's
 * capacity are clamped by the kernels; every such event is counted.  Call after synchronising the stream(s) the launches
 * went to: *count = events so far (sticky), returns DVM_ERR_CAPACITY if non-zero. */
int dvm_frame_overflows(dvm_frame* f, int32_t* count);

typedef struct {
  int32_t best_idx;     /* index into the slot's ORIGINAL keypoint order, -1 if no candidate */
  int32_t best_dist;    /* 256 if none */
  int32_t second_dist;  /* 256 if none */
  int16_t best_level, second_level; /* octaves of best / second best, -1 if none */
} dvm_match;

/* For each query q: scan Frame::GetFeaturesInArea(qx,qy,qr,qmin,qmax) of train slot `slot`
 * (skipping indices with skip[idx]!=0, skip may be NULL) and return best / second best by
 * DescriptorDistance with the reference's strict-'<' first-wins tie rule.  Query arrays: qdesc
 * nq x 32 B, qx/qy/qr float, qmin/qmax int32 (-1 = unbounded, as in the reference).  d_nq (device
 * int32*, may be NULL) overrides nq.  All pointers are device pointers when on_device != 0
 * (asynchronous on `stream`), else host pointers (synchronous). */
int dvm_match_window(const dvm_frame* train, int slot, const uint8_t* skip, const uint8_t* qdesc, const float* qx,
                     const float* qy, const float* qr, const int32_t* qmin, const int32_t* qmax, int nq,
                     const int32_t* d_nq, dvm_match* out, int on_device, void* stream);
/* The same search, also returning the runner-up's train index (second_idx[q], -1 if none; may be NULL): what the reference's
 * scan returns when the best candidate is excluded -- a caller replaying ORBmatcher.cc:1613-1664's claims in query order takes
 * it when the best candidate was claimed by an earlier query of the same call, instead of searching again. */
int dvm_match_window_top2(const dvm_frame* train, int slot, const uint8_t* skip, const uint8_t* qdesc, const float* qx,
                          const float* qy, const float* qr, const int32_t* qmin, const int32_t* qmax, int nq,
                          const int32_t* d_nq, dvm_match* out, int32_t* second_idx, int on_device, void* stream);
/* The same scan returning the FOUR best candidates of every query in the reference's order of preference (distance, then scan
 * position): ranked[4 q + c] = dist << 16 | train index, dist = 256 from the end of the list on (fewer than four candidates: the list
 * is complete).  For a caller replaying ORBmatcher.cc:1613-1664's claims in query order: it walks the list to the first keypoint no
 * earlier query of the call has taken, and searches again itself only when all four are gone. */
int dvm_match_window_ranked(const dvm_frame* train, int slot, const uint8_t* skip, const uint8_t* qdesc, const float* qx, const float* qy,
                            const float* qr, const int32_t* qmin, const int32_t* qmax, int nq, uint32_t* ranked, int on_device, void* stream);
/* Host-pointer convenience, latency path of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame) (ORBmatcher.cc:1553-1748):
 * dvm_frame_build(f, slot, kps, desc, n, ..., on_device = 0) followed by dvm_match_window_ranked(f, slot, ..., on_device = 0) as ONE
 * staged call -- one upload, the two kernels back to back on the calling thread's stream, one synchronisation.  Same results as
 * the two calls.  kps_on_device != 0: kps / desc are DEVICE arrays (dvm_orb_last_result: the frame as the extractor left it in HBM);
 * everything else stays a host pointer. */
int dvm_frame_build_match_window_ranked(dvm_frame* f, int slot, const dvm_keypoint* kps, const uint8_t* desc, int n, float minX,
                                        float maxX, float minY, float maxY, const uint8_t* skip, const uint8_t* qdesc,
                                        const float* qx, const float* qy, const float* qr, const int32_t* qmin,
                                        const int32_t* qmax, int nq, uint32_t* ranked, int kps_on_device);
/* The shared form of the call above for several agents on one GPU (as dvm_orb_pool for the extractor): the same arguments (host pointers), the
 * same ranked lists, callable from any number of threads; calls that arrive within `window_us` of each other and share the image bounds run
 * as ONE launch pair over the batch's grid slots.  kp_cap / q_cap: keypoints / queries per frame the pool holds (a larger frame is refused
 * with DVM_ERR_CAPACITY: the caller takes dvm_frame_build_match_window_ranked).  batch_size (may be NULL): frames in the call's launch. */
typedef struct dvm_match_pool dvm_match_pool;
int dvm_match_pool_create(int device, int max_batch, int kp_cap, int q_cap, int window_us, dvm_match_pool** out);
void dvm_match_pool_destroy(dvm_match_pool* pool);
int dvm_match_pool_capacity(const dvm_match_pool* pool, int* kp_cap, int* q_cap);
int dvm_match_pool_build_match_ranked(dvm_match_pool* pool, const dvm_keypoint* kps, const uint8_t* desc, int n, float minX, float maxX, float minY,
                                      float maxY, const uint8_t* skip, const uint8_t* qdesc, const float* qx, const float* qy, const float* qr,
                                      const int32_t* qmin, const int32_t* qmax, int nq, uint32_t* ranked, int* batch_size);
/* The stream the host-pointer convenience calls of the CALLING THREAD run on (device `device`; created on first use).  A caller
 * that builds a grid with on_device = 1 and then searches it through a host-pointer call passes it as `stream`, so that the two are
 * one in-order chain (no synchronisation in between). */
void* dvm_thread_stream(int device);

/* Frame::UndistortKeyPoints (Frame.cc:791-818) and Frame::ComputeImageBounds (:820-848): cv::undistortPoints(pts, K, D,
 * noArray(), K) -- OpenCV's 5-iteration fixed-point inversion of the (k1, k2, p1, p2, k3) model, in double from the float
 * inputs.  kps_out[i] = kps_in[i] with the point replaced (in place allowed); k1 == 0 copies, as the reference's early return
 * does.  dvm_image_bounds: {mnMinX, mnMaxX, mnMinY, mnMaxY} from the four undistorted image corners ({0, cols, 0, rows} for
 * k1 == 0); the values dvm_frame_build and the matcher gates take.  Host pointers (synchronous) or device pointers. */
typedef struct { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } dvm_distortion;
int dvm_undistort_keypoints(const dvm_distortion* cam, const dvm_keypoint* kps_in, dvm_keypoint* kps_out, int n, int on_device, void* stream);
int dvm_image_bounds(const dvm_distortion* cam, int cols, int rows, float bounds[4]);

/* Frame::isInFrustum (Frame.cc:575-636, mono branch) for n map points at once: projection with the frame's
 * Rcw/tcw (float; mRcw = mTcw.rotationMatrix(), Frame.cc:553-559 -- this function does use the matrix form, :585),
 * image bounds, distance inside [0.8*mfMinDistance, 1.2*mfMaxDistance], viewing cosine,
 * MapPoint::PredictScale.  Outputs the mbTrackInView / mTrackProj* / mnTrackScaleLevel / mTrackViewCos fields the
 * reference stores on the MapPoint.  Host pointers (synchronous) or device pointers (asynchronous on `stream`). */
typedef struct { float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, min_x, max_x, min_y, max_y, bf, log_scale_factor; int32_t n_levels; } dvm_frustum_frame;
typedef struct { float proj_x, proj_y, proj_xr, depth, view_cos; int32_t level; int32_t in_view; } dvm_track_point;
int dvm_is_in_frustum(const dvm_frustum_frame* frame, const float* P, const float* normal, const float* min_dist,
                      const float* max_dist, int n, float viewing_cos_limit, dvm_track_point* out, int on_device, void* stream);

/* A camera model of the reference's GeometricCamera (CameraModels/Pinhole.cpp, KannalaBrandt8.cpp), evaluated by csrc/camera_model.h.
 * KannalaBrandt8: theta = atan2(sqrt(x^2 + y^2), z), r = theta + k1 theta^3 + k2 theta^5 + k3 theta^7 + k4 theta^9,
 * u = fx r x / rho + cx, v = fy r y / rho + cy (rho = sqrt(x^2 + y^2); on the optical axis u = cx, v = cy).  Its Jacobian
 * (projectJac, KannalaBrandt8.cpp:144-172) is 0 / 0 on the optical axis: NaN there, as in the reference.  sizeof(dvm_camera_model) == 36.
 * Every *_cam entry returns DVM_ERR_INVALID, before anything runs, for a NULL model, a model outside {0, 1} or a zero focal length.
 * What takes a model: dvm_pose_optimize_cam, dvm_is_in_frustum_cam, dvm_project_search_cam, dvm_ba_set_problem_cam,
 * dvm_ba_optimize_windows_fast_cam, dvm_ba_pool_optimize_cam, dvm_match_triangulation_cam, dvm_triangulate_matches_cam, dvm_create_new_map_points_cam,
 * dvm_sim3_hypotheses_cam, dvm_optimize_sim3_cam (and dvmh_search_by_projection_frames_cam,
 * dvmh_triangulation_geometry_cam, dvmh_search_for_triangulation_cam, dvmh_create_new_map_points_cam, include/dvmslam_host.h).  The
 * entries that take the models of TWO keyframes want one model type for both (the parameters may differ per keyframe): a pair of a
 * pinhole and a KannalaBrandt8 keyframe is DVM_ERR_INVALID -- the reference's mixed pair is out of scope -- except the two Sim3 entries
 * (dvm_sim3_hypotheses_cam, dvm_optimize_sim3_cam), which take all four pairs: a merge between a pinhole and a fisheye agent.  The tracked-frame
 * chains take the agent's model as state of the tracker (dvm_tracker_set_camera_model below).  The pools (dvm_orb_pool_*, dvm_match_pool_*,
 * dvm_pose_pool_*), the BoW chain, the sequential-order BA windows (dvm_ba_optimize_windows), dvm_ba_optimize_batch,
 * dvm_ba_set_problem_sharded, two-view initialisation and the Sim3Solver / Optimizer shim classes (include/dvmslam_host.h) are pinhole-only. */
typedef struct { int32_t model;   /* 0 pinhole, 1 KannalaBrandt8 */
                 float p[8];      /* fx, fy, cx, cy, k1, k2, k3, k4: mvParameters, float as the reference stores them */
} dvm_camera_model;
/* dvm_is_in_frustum with uv = mpCamera->project(Pc) (Frame.cc:594) of `model`: model->p[0..3] replace frame->fx, fy, cx, cy, which are
 * not read.  Everything else, proj_xr = u - bf * invz included, as in dvm_is_in_frustum; model 0 gives its results bit for bit.  A
 * KannalaBrandt8 monocular frame has mvKeysUn = mvKeys and bounds 0 .. cols / 0 .. rows (mDistCoef is zero): the caller passes those. */
int dvm_is_in_frustum_cam(const dvm_frustum_frame* frame, const dvm_camera_model* model, const float* P, const float* normal,
                          const float* min_dist, const float* max_dist, int n, float viewing_cos_limit, dvm_track_point* out, int on_device,
                          void* stream);

/* LocalMapping::CreateNewMapPoints, the geometry of ONE neighbour keyframe (LocalMapping.cc:598-741, monocular pinhole branch) for
 * the index pairs ORBmatcher::SearchForTriangulation returned: unprojectEig, parallax of the two rays (cos > 0 and, in double,
 * < cos_parallax_max: 0.9998, 0.9996 inertial), GeometricTools::Triangulate (GeometricTools.cc:48-67), z > 0 in both cameras,
 * reprojection error <= 5.991 * mvLevelSigma2[octave] in both, zero / far distance, the distance-ratio vs octave-ratio test with
 * ratio_factor = 1.5f * mfScaleFactor.  pairs[2 m], pairs[2 m + 1] = index into kps1 (the current keyframe's mvKeysUn) / kps2.
 * x3D[3 m ..] = the triangulated point (zeros when no triangulation was attempted), status[m]: 0 accepted -- the caller creates the
 * MapPoint --, 1 parallax, 2 homogeneous w == 0, 3 z1 <= 0, 4 z2 <= 0, 5 / 6 reprojection error in keyframe 1 / 2, 7 zero distance,
 * 8 far point, 9 scale consistency, -1 index or octave out of range.  float arithmetic in Eigen's evaluation order; the null
 * vector of the 4x4 system comes from a double Jacobi diagonalisation of A^T A instead of Eigen::JacobiSVD<Matrix4f> (tolerance
 * parity on x3D).  Host pointers (synchronous) or device pointers (asynchronous on `stream`). */
typedef struct {
  double cos_parallax_max;
  float K1[4], K2[4];       /* fx, fy, cx, cy */
  float T1w[12], T2w[12];   /* KeyFrame::GetPose().matrix3x4(), row-major */
  float Ow1[3], Ow2[3];     /* KeyFrame::GetCameraCenter() */
  float ratio_factor, th_far;
  int32_t far_points;       /* mbFarPoints */
  int32_t n_levels;         /* length of the sigma2 / scale-factor tables */
} dvm_tri_pair;
int dvm_triangulate_matches(const dvm_tri_pair* pair, const dvm_keypoint* kps1, int n1, const dvm_keypoint* kps2, int n2,
                            const int32_t* pairs, int n, const float* sigma2_1, const float* sigma2_2, const float* scale_factors_1,
                            const float* scale_factors_2, float* x3D, int32_t* status, int on_device, void* stream);

/* The relative pose of a keyframe pair as SearchForTriangulation holds it -- T12 = T1w * Tw2, R12 = T12.rotationMatrix(), t12 =
 * T12.translation() (ORBmatcher.cc:856-859; dvmh_triangulation_geometry computes both) -- and what KannalaBrandt8::TriangulateMatches
 * derives from it for every candidate (KannalaBrandt8.cpp:335-336): R21 = R12^T, t21 = -R21 t12.  dvm_pair_pose_set fills all four from
 * R12 and t12, once per pair, on the host (index-free float arithmetic in Eigen's order). */
typedef struct { float R12[9], t12[3], R21[9], t21[3]; } dvm_pair_pose;
void dvm_pair_pose_set(const float* R12, const float* t12, dvm_pair_pose* out);

/* dvm_triangulate_matches on a camera model per keyframe: xn = pCamera->unprojectEig(kp.pt) and both reprojection errors from
 * pCamera->project(Point3f(x, y, z)) (LocalMapping.cc:608-609, :676, :700); the parallax gate, GeometricTools::Triangulate with its
 * w == 0 test, the depth, distance and scale-consistency tests and the status codes are dvm_triangulate_matches'.  model1 / model2 = the
 * cameras of kps1 / kps2; their p[0..3] replace pair->K1 / K2, which are not read.  Both models of one type (else DVM_ERR_INVALID);
 * model 0 gives dvm_triangulate_matches' results bit for bit. */
int dvm_triangulate_matches_cam(const dvm_tri_pair* pair, const dvm_camera_model* model1, const dvm_camera_model* model2, const dvm_keypoint* kps1,
                                int n1, const dvm_keypoint* kps2, int n2, const int32_t* pairs, int n, const float* sigma2_1, const float* sigma2_2,
                                const float* scale_factors_1, const float* scale_factors_2, float* x3D, int32_t* status, int on_device, void* stream);

/* Best / second best over an explicit candidate list per query -- the inner loop of the
 * vocabulary-node restricted searches (SearchByBoW ORBmatcher.cc:262-300,760-800; SearchForTriangulation
 * :905-960; SearchBySim3; Fuse): query q scans train descriptors cand[off[q] .. off[q+1]) in that order
 * (entries < 0 are skipped), strict-'<' first-wins.  best_idx is the train index, levels are -1.
 * Host pointers (synchronous) or device pointers (asynchronous on `stream`). */
int dvm_match_lists(const uint8_t* tdesc, int nt, const uint8_t* qdesc, int nq, const int32_t* off, const int32_t* cand,
                    dvm_match* out, int on_device, void* stream);

/* Projection of n map points into a keyframe + windowed best-descriptor search -- the common body of
 * ORBmatcher::Fuse(KF, vpMapPoints, th) (ORBmatcher.cc:1060-1234, gate_inv_sigma2 = KF.mvInvLevelSigma2, gate = 5.99),
 * Fuse(KF, Scw, ...) (:1236-1345), SearchByProjection(KF, Scw, vpPoints, vpMatched, th, ratioHamming) x2 (:395-603),
 * both directions of SearchBySim3 (:1347-1551; cam->sim3_pair) (gate_inv_sigma2 = NULL).  Per point (skipped when valid[i] == 0; valid may be NULL):
 * p3Dc = Tcw * p in Sophus' QUATERNION form (Thirdparty/Sophus/sophus/so3.hpp:356-367, se3.hpp:319-324 -- the reference never
 * goes through a rotation matrix here, and the two forms differ in the last float ulp), depth >= 0, KeyFrame::IsInImage,
 * dist in [0.8*min_dist, 1.2*max_dist], PO.Pn >= 0.5*dist, level = MapPoint::PredictScale, radius = th *
 * scale_factors[level], candidates = KeyFrame::GetFeaturesInArea(u, v, radius) with octave in [level-1, level], minus
 * skip[idx] != 0 (skip may be NULL; `cap` bytes of the train frame).  out[i] = best / second best (strict '<', first
 * wins); proj[i] (may be NULL) = projection, radius and predicted level (-1: rejected before the search).
 * Host pointers (synchronous) or device pointers (asynchronous on `stream`). */
typedef struct { float q[4], t[3]; } dvm_se3f;   /* Sophus::SE3f: unit_quaternion().coeffs() = (x, y, z, w), translation() */
typedef struct { float q[4], t[3]; } dvm_sim3f;  /* Sophus::Sim3f: rxso3().quaternion().coeffs() (scale = |q|^2), translation() */
typedef struct {
  /* Tcw: KeyFrame::GetPose() / Frame::GetPose(); for the Sim3 variants SE3f(Scw.rotationMatrix(), Scw.translation() /
   * Scw.scale()) (ORBmatcher.cc:403,505,1245 -- dvm_host::Sim3ToSE3 derives it in the reference's order).
   * Ow: GetCameraCenter() resp. Tcw.inverse().translation(). */
  dvm_se3f Tcw;
  float Ow[3], fx, fy, cx, cy, min_x, max_x, min_y, max_y, log_scale_factor;
  int32_t n_levels;
  /* sim3_pair == 1 selects the ORBmatcher::SearchBySim3 form (ORBmatcher.cc:1380-1437): p' = S2 * (Tcw * p) with Tcw the
   * OTHER keyframe's pose and S2 = S21 resp. S12 (Sim3f action rxso3.hpp:265-273, sim3.hpp:226-229),
   * u = fx * (X * invz) + cx with invz = 1.0 / Z, distance = |p'|, no viewing-angle test; Ow is not used.
   * sim3_pair == 2 selects the relocalisation form, ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th,
   * ORBdist) (:1750-1860): no depth test, bounds inclusive at both ends, no viewing-angle test, octaves [level-1, level+1]. */
  int32_t sim3_pair;
  dvm_sim3f S2;
} dvm_kf_camera;
typedef struct { float u, v, radius; int32_t level; } dvm_projection;
int dvm_project_search(const dvm_frame* train, int slot, const uint8_t* skip, const dvm_kf_camera* cam, const float* P,
                       const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc,
                       const uint8_t* valid, int n, float th, const float* scale_factors, const float* gate_inv_sigma2,
                       double gate, dvm_match* out, dvm_projection* proj, int on_device, void* stream);
/* dvm_project_search with uv = pCamera->project(p3Dc) of `model` (ORBmatcher.cc:431, :1117, :1274, :1774): model->p[0..3] replace
 * cam->fx, fy, cx, cy, which are not read.  The chi2 gate of Fuse(KF, vpMapPoints) takes its error from that u, v; nothing else about it
 * changes.  cam->sim3_pair == 1 (SearchBySim3) keeps u = fx * (X * invz) + cx: the reference writes the pinhole formula inline there
 * (ORBmatcher.cc:1401-1406) whatever the camera, so that form reads p[0..3] only.  Model 0 gives dvm_project_search's results bit for bit. */
int dvm_project_search_cam(const dvm_frame* train, int slot, const uint8_t* skip, const dvm_kf_camera* cam, const dvm_camera_model* model,
                           const float* P, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc,
                           const uint8_t* valid, int n, float th, const float* scale_factors, const float* gate_inv_sigma2, double gate,
                           dvm_match* out, dvm_projection* proj, int on_device, void* stream);

/* ORBmatcher::SearchForTriangulation inner loop (ORBmatcher.cc:905-998, monocular): query q = keypoint qidx[q] of KF1
 * scans the KF2 keypoints cand[off[q] .. off[q+1]) (entries < 0 skipped); a candidate is kept if dist <= 50, dist <= best
 * so far, it is not within sqrt(100*scale_factors2[octave]) px of the epipole `ep`, and (coarse != 0 or)
 * Pinhole::epipolarConstrain (CameraModels/Pinhole.cpp:104-127) holds with the fundamental matrix F12 (row-major 3x3,
 * float) and level_sigma2_2[octave].  best_idx[q] = KF2 index (-1 none), best_dist[q] (256 none); a tie goes to the LAST
 * candidate, as the reference's "dist > bestDist -> continue" does. */
int dvm_match_triangulation(const uint8_t* desc1, const dvm_keypoint* kps1, int n1, const int32_t* qidx, int nq,
                            const uint8_t* desc2, const dvm_keypoint* kps2, int n2, const int32_t* off, const int32_t* cand,
                            const float* F12, const float* ep, int coarse, const float* scale_factors2,
                            const float* level_sigma2_2, int nlevels, int32_t* best_idx, int32_t* best_dist, int on_device,
                            void* stream);

/* dvm_match_triangulation on a camera model per keyframe.  Under KannalaBrandt8 the candidate test after dist <= 50 and the epipole disc
 * is KannalaBrandt8::epipolarConstrain (KannalaBrandt8.cpp:216-220): TriangulateMatches (:304-374) > 0.0001f, all in float -- the two rays
 * (unproject), their parallax against the double 0.9998, the point from the 4x4 system of cameras [I | 0] and [R21 | t21] (null vector by
 * the double Jacobi of A^T A; division by the fourth component with no w == 0 test), z > 0 in both cameras, the reprojection error through
 * project() of camera 1 against 5.991 * level_sigma2_1[kp1.octave] and of camera 2 against 5.991 * level_sigma2_2[kp2.octave]; the value
 * is z1.  It reads KF1's level_sigma2 beside KF2's; F12 is not read (may be NULL) and `ep` is the caller's
 * pKF2->mpCamera->project(T2w * Cw) (dvmh_triangulation_geometry_cam).  A candidate whose octave lies outside [0, nlevels) is no
 * candidate; a query whose octave does finds nothing unless coarse != 0.  Under model 0 `pose` and level_sigma2_1 are not read (may be
 * NULL) and the results are dvm_match_triangulation's bit for bit.  Both models of one type (else DVM_ERR_INVALID). */
int dvm_match_triangulation_cam(const uint8_t* desc1, const dvm_keypoint* kps1, int n1, const int32_t* qidx, int nq, const uint8_t* desc2,
                                const dvm_keypoint* kps2, int n2, const int32_t* off, const int32_t* cand, const dvm_camera_model* model1,
                                const dvm_camera_model* model2, const dvm_pair_pose* pose, const float* F12, const float* ep, int coarse,
                                const float* level_sigma2_1, const float* scale_factors2, const float* level_sigma2_2, int nlevels,
                                int32_t* best_idx, int32_t* best_dist, int on_device, void* stream);

/* LocalMapping::CreateNewMapPoints (LocalMapping.cc:446-760, monocular; pinhole here, any model through the _cam entry below) for ALL neighbour keyframes of the current keyframe as
 * ONE device chain: one upload, three launches whatever n_neighbours is, one synchronisation.  Per neighbour, in the order given:
 *   1. baseline test (:497-512): baseline = ||Ow2 - Ow1|| in float, summed as x^2 + y^2 + z^2; ratio = baseline / median_depth in float;
 *      the neighbour is skipped when (double)ratio < 0.01 -- plain arithmetic, no special case: a negative median depth (what
 *      ComputeSceneMedianDepth returns without points) skips, a zero one gives +inf and does not;
 *   2. ORBmatcher::SearchForTriangulation (what dvm_match_triangulation + the host's node walk and rotation check do today) against the
 *      current keyframe's map-point table AS THE EARLIER NEIGHBOURS LEFT IT;
 *   3. the geometry of dvm_triangulate_matches for every pair the search returned (same codes, same zero-filling);
 *   4. every KF1 keypoint of a status-0 pair is marked as having a point.
 * The reference never sets vbMatched2 (ORBmatcher.cc:878,927), so the best KF2 candidate of a KF1 keypoint depends on that keypoint and the
 * neighbour only: the search and the geometry of all (neighbour, keypoint without a point at entry) run speculatively in two launches, and
 * one workgroup then walks the neighbours in order -- live matches (no point so far), rotation histogram + ComputeThreeMaxima over them,
 * compaction in ascending idx1, table update.  The results equal the loop of the separate calls bit for bit.
 *
 * dvm_np_keyframe: what the two separate calls read of a keyframe.  mp[i] = map point id of keypoint i, -1 = none (of a neighbour: KF2
 * features with a point are no candidates).  fv_*: the flattened DBoW2::FeatureVector (dvmh_feature_vector_view): node ids strictly
 * ascending -- FeatureVector nodes ascend as unsigned; -1 is last (dvmslam_host.h) --, features of node k = fv_feat[fv_off[k] .. fv_off[k+1]), fv_off[0] = 0, at most n features in all.  A neighbour also carries
 * median_depth = ComputeSceneMedianDepth(2) (the map points live with the caller) and the pair geometry ep / F12 as
 * dvmh_triangulation_geometry(cur, neighbour) computes it (index-free host arithmetic; dvmh_create_new_map_points fills it in).
 * PRECONDITION: the neighbours are distinct keyframes (GetBestCovisibilityKeyFrames returns each once; a data-only check cannot see it).
 *
 * dvm_np_out (caller memory, written once after the synchronisation):
 *   nb_status[n_neighbours]   0 ran, 1 skipped by the baseline test
 *   nb_matches[n_neighbours]  SearchForTriangulation's return value for that neighbour (0 when skipped)
 *   pair_off[n_neighbours+1]  neighbour j's records are [pair_off[j], pair_off[j+1])
 *   pairs[2 m], status[m], x3D[3 m]   flat records in neighbour order, inside a neighbour by ascending idx1 -- exactly vMatchedIndices;
 *                             ALL pairs are recorded, not only the accepted ones; record_cap = records the three arrays hold
 *   new_point[cur->n]         the record that gave KF1 keypoint i its point, -1 none
 * How a caller that honours CheckNewKeyFrames() (:490) uses it: the records of neighbour j do not depend on later neighbours, so it applies
 * the records neighbour by neighbour and stops at the neighbour at which the reference would have returned; the rest is dropped.  Two records
 * of one neighbour may name the same idx2 (both status 0): they come in idx1 order and the caller's pKF2->AddMapPoint overwrites, as the
 * reference's does.
 *
 * Errors, all reported before anything runs and leaving the handle usable: DVM_ERR_CAPACITY -- cur->n, n_neighbours or the neighbours'
 * total keypoints beyond the reservation, or record_cap < n_neighbours x (keypoints of cur without a point); DVM_ERR_INVALID -- a keyframe
 * with n > 8192, non-monotone fv_off, a feature index outside [0, n), nodes not ascending, level tables of unequal length or outside
 * [1, 64], a zero focal length, a missing array, p->monocular != 1 (the stereo branches are outside the project's scope, as in the
 * separate calls).  A KF2 candidate whose octave lies outside the tables is no candidate; a KF1 keypoint whose octave does gives status -1
 * with nothing read.  dvm_new_points_create returns DVM_ERR_NO_DEVICE without a GPU. */
typedef struct {
  int32_t n;
  const dvm_keypoint* kps;      /* mvKeysUn */
  const uint8_t* desc;          /* n x 32 */
  const int32_t* mp;            /* n */
  int32_t fv_n;
  const int32_t *fv_node, *fv_off, *fv_feat;
  dvm_se3f Tcw, Twc;            /* GetPose(), GetPoseInverse() */
  float Ow[3];                  /* GetCameraCenter() */
  float fx, fy, cx, cy;
  const float* scale_factors;   /* mvScaleFactors */
  const float* level_sigma2;    /* mvLevelSigma2 */
  int32_t n_levels;
} dvm_np_keyframe;
typedef struct {
  dvm_np_keyframe kf;
  float median_depth;
  float ep[2], F12[9];
} dvm_np_neighbour;
typedef struct {
  double cos_parallax_max;      /* 0.9998, 0.9996 inertial (:655-656) */
  float ratio_factor;           /* 1.5f * mpCurrentKeyFrame->mfScaleFactor (:483) */
  float th_far;                 /* mThFarPoints */
  int32_t far_points;           /* mbFarPoints */
  int32_t coarse, check_ori;    /* bCoarse; the matcher's mbCheckOrientation */
  int32_t monocular;            /* must be 1 */
} dvm_np_params;
typedef struct {
  int32_t *nb_status, *nb_matches, *pair_off;
  int32_t* pairs;
  int32_t* status;
  float* x3D;
  int32_t* new_point;
  int32_t record_cap;
} dvm_np_out;
typedef struct dvm_new_points dvm_new_points;
int dvm_new_points_create(int device, dvm_new_points** out);
void dvm_new_points_destroy(dvm_new_points* h);
/* the working set for calls up to these sizes (grow-only; a call never allocates) */
int dvm_new_points_reserve(dvm_new_points* h, int max_kf1_keypoints, int max_neighbours, int max_total_neighbour_keypoints);
int dvm_create_new_map_points(dvm_new_points* h, const dvm_np_keyframe* cur, int n_neighbours, const dvm_np_neighbour* nbs,
                              const dvm_np_params* p, dvm_np_out* out);
/* dvm_create_new_map_points on a camera model per keyframe: cur_model = the current keyframe's camera, nb_models[j] / nb_poses[j] =
 * neighbour j's camera and the pair's relative pose (dvm_pair_pose_set).  The models' p[0..3] replace the keyframes' fx, fy, cx, cy,
 * which are not read.  Under KannalaBrandt8 the search is dvm_match_triangulation_cam's and the geometry dvm_triangulate_matches_cam's;
 * nbs[j].ep is the epipole through neighbour j's model and nbs[j].F12 is not read.  Three launches, as the pinhole chain: every ray is
 * taken where it is used (a pre-pass that wrote all rays into a table first was measured and was no faster).  The records equal the loop
 * of the two _cam calls bit for bit.  Under model 0 nb_poses is not read (may be NULL) and the call is
 * dvm_create_new_map_points.  All models of one type: a NULL model, a model outside {0, 1}, a zero focal length or a mixed pair is
 * DVM_ERR_INVALID before anything runs, and the handle stays usable.  A KF1 keypoint whose octave lies outside the tables finds nothing
 * in a KannalaBrandt8 search unless p->coarse (under model 0 it is matched and gets status -1). */
int dvm_create_new_map_points_cam(dvm_new_points* h, const dvm_np_keyframe* cur, const dvm_camera_model* cur_model, int n_neighbours,
                                  const dvm_np_neighbour* nbs, const dvm_camera_model* nb_models, const dvm_pair_pose* nb_poses,
                                  const dvm_np_params* p, dvm_np_out* out);
/* HIP-event timing of the three launches (measurement only): enable != 0 makes every call record events; ms[3] = search, geometry,
 * settle of the last call that ran */
int dvm_new_points_profiling(dvm_new_points* h, int enable);
int dvm_new_points_last_kernel_ms(dvm_new_points* h, float* ms);

/* The first half of LocalMapping::SearchInNeighbors (LocalMapping.cc:812-821): ORBmatcher::Fuse(pKFi, vpMapPointMatches) once per target
 * keyframe -- its search part (ORBmatcher.cc:1089-1210) for ALL targets as ONE chain.  The search reads the target keyframe, the point's
 * position, normal, distance range and descriptor, and two skip conditions (isBad(), IsInKeyFrame(pKF)); everything the loop mutates is in
 * the apply step (:1213-1228), which stays with the caller.  Walking the targets in order moves only three things: isBad() and
 * IsInKeyFrame(target) can only turn true (a host-side skip when the row is applied), and MapPoint::Replace ends in
 * ComputeDistinctiveDescriptors (MapPoint.cc:356), so a surviving point may carry a new descriptor for the later targets.  All T x n searches
 * therefore run speculatively in one launch, and the caller runs again -- masked -- the rows of points whose descriptor really changed.
 *
 *   set   uploads all targets in one staged copy and builds all their grids in one launch (the order dvm_frame_build produces, the spans
 *         back to back).  It does not wait.  The targets stay resident until the next set (or a reserve that grows the working set).
 *   run   uploads the point table and the mask once, launches ONE kernel over (target, point) -- one 16-lane row per pair -- and copies the
 *         two result arrays back behind one synchronisation.  It may be called again on the same targets with other points or masks.
 *
 * Contract: best_idx / best_dist [T * n], entry (t, i) at t * n + i, equals bit for bit what dvm_project_search returns for target t alone
 * with gate_inv_sigma2 = inv_level_sigma2, gate = 5.99 and valid[i] && !skip[t * n + i]; then dvmh_fuse's rule: best_idx = -1 unless
 * best_dist <= 50 (ORBmatcher::TH_LOW).  best_dist (may be NULL) is the raw distance, 256 without a candidate.  A masked entry costs its
 * row's early exit and reads best_idx = -1, best_dist = 256.
 *
 * Errors, all reported before anything runs and leaving the handle (and the resident targets) usable: DVM_ERR_CAPACITY -- targets, their
 * total keypoints or the points beyond the reservation; DVM_ERR_INVALID -- a target with n > 8192, n_levels outside [1, 64], a zero focal
 * length, empty image bounds, a keypoint whose octave lies outside the level tables (the gate indexes them), a missing array, run before
 * set.  dvm_fuse_targets_create returns DVM_ERR_NO_DEVICE without a GPU.  A target with n = 0 is legal (all its entries are -1 / 256);
 * n_targets = 0 and P->n = 0 are legal and write nothing.  sizeof(dvm_ft_target) == 120, sizeof(dvm_ft_points) == 56 (LP64). */
typedef struct {
  int32_t n;
  const dvm_keypoint* kps;          /* mvKeysUn */
  const uint8_t* desc;              /* n x 32 */
  dvm_se3f Tcw;                     /* GetPose() */
  float Ow[3];                      /* GetCameraCenter() */
  float fx, fy, cx, cy;
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  const float* scale_factors;       /* mvScaleFactors */
  const float* inv_level_sigma2;    /* mvInvLevelSigma2 */
  float log_scale_factor;           /* mfLogScaleFactor */
  int32_t n_levels;
} dvm_ft_target;
typedef struct {
  int32_t n;
  const float* pos;                 /* 3n  GetWorldPos() */
  const float* normal;              /* 3n  GetNormal() */
  const float* min_dist;            /* mfMinDistance, mfMaxDistance: the search applies the factors 0.8f / 1.2f */
  const float* max_dist;
  const uint8_t* desc;              /* 32n GetDescriptor() */
  const uint8_t* valid;             /* n; may be NULL (all valid) */
} dvm_ft_points;
typedef struct dvm_fuse_targets dvm_fuse_targets;
int dvm_fuse_targets_create(int device, dvm_fuse_targets** out);
void dvm_fuse_targets_destroy(dvm_fuse_targets* h);
/* the working set for calls up to these sizes (grow-only; set and run never allocate).  Growing it drops the resident targets. */
int dvm_fuse_targets_reserve(dvm_fuse_targets* h, int max_points, int max_targets, int max_total_target_keypoints);
int dvm_fuse_targets_set(dvm_fuse_targets* h, int n_targets, const dvm_ft_target* targets);
int dvm_fuse_targets_run(dvm_fuse_targets* h, const dvm_ft_points* P, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist);
/* HIP-event timing (measurement only): enable != 0 makes set and run record events; ms[2] = grid build of the last set, search of the
 * last run (read after a run) */
int dvm_fuse_targets_profiling(dvm_fuse_targets* h, int enable);
int dvm_fuse_targets_last_kernel_ms(dvm_fuse_targets* h, float* ms);
/* dvm_fuse_targets_set with a camera model and a form PER TARGET (dvm_camera_model above).
 *   models [n_targets], or NULL: every target projects with its own fx, fy, cx, cy.  models[t] is target t's pKF->mpCamera: under model 1 the
 *          projection is dvm_cam::kb8_project on models[t].p and targets[t].fx .. cy are not read -- the rule of dvm_project_search_cam.
 *          Targets of both model types may be mixed in one call (rows are independent; after a merge an agent's map holds keyframes of
 *          other agents' cameras).
 *   forms  [n_targets], or NULL: all DVM_FT_FORM_POINTS.  Under DVM_FT_FORM_SCW targets[t].Tcw and Ow are what dvm_host::Sim3ToSE3(Scw)
 *          derives (as for dvm_project_search), inv_level_sigma2 is not read and may be NULL, and acceptance stays best_dist <= 50.
 * Contract: row t of a run equals bit for bit what dvm_project_search_cam returns for target t alone with that target's model,
 * gate_inv_sigma2 = forms[t] ? NULL : inv_level_sigma2, gate = 5.99 and valid[i] && !skip[t * n + i], followed by the <= 50 rule.
 * dvm_fuse_targets_set(h, n, targets) is dvm_fuse_targets_set_cam(h, n, targets, NULL, NULL).
 * Errors: those of dvm_fuse_targets_set, in both forms (the zero focal length of the target's own fx, fy only where no model is given; a
 * missing inv_level_sigma2 only under DVM_FT_FORM_POINTS), and DVM_ERR_INVALID for a model outside {0, 1}, a zero focal length of a given
 * model, or a form outside {0, 1}; each names the target, is reported before anything runs and leaves the handle and its resident
 * targets usable. */
#define DVM_FT_FORM_POINTS 0  /* Fuse(pKF, vpMapPoints, th): the 5.99 gate on inv_level_sigma2 */
#define DVM_FT_FORM_SCW    1  /* Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) search part (ORBmatcher.cc:1256-1330): no chi2 gate */
int dvm_fuse_targets_set_cam(dvm_fuse_targets* h, int n_targets, const dvm_ft_target* targets,
                             const dvm_camera_model* models /* [n_targets], or NULL: the targets' fx, fy, cx, cy */,
                             const uint8_t* forms /* [n_targets], or NULL: all DVM_FT_FORM_POINTS */);
/* The hits of a run instead of its dense rows (LoopClosing::SearchAndFuse sizes: over a hundred keyframes x thousands of points, of which
 * a few thousand entries are hits).  The search kernel writes its dense rows to device memory as dvm_fuse_targets_run does; a stable
 * compaction (count per target, scan over the targets, write -- three launches, no workgroup waits on another) then writes hit_off and the
 * hits into a mapped page-locked block, and ONE synchronisation follows.  Nothing of size T x n comes back to the host.
 *   hits[hit_off[t] .. hit_off[t + 1]) are target t's entries with best_idx >= 0, in ascending point, with the idx and dist that
 *   dvm_fuse_targets_run returns on the same inputs; *n_hits (may be NULL) is the total = hit_off[T].
 * dvm_fuse_targets_reserve_hits: the block for up to max_hits hits (grow-only; a dvm_fuse_targets_reserve that grows keeps it).
 * dvm_fuse_targets_run_hits before it is DVM_ERR_INVALID.  A total beyond hit_cap or the reservation: DVM_ERR_CAPACITY; *n_hits and hit_off
 * still hold the full counts (the caller sizes a repeat from them), hits is unspecified, the device has written nothing past its block
 * (the write kernel checks every position) and the handle stays usable.  T = 0 and P->n = 0 write hit_off (all zero) and *n_hits = 0.
 * sizeof(dvm_ft_hit) == 12. */
typedef struct { int32_t point, idx, dist; } dvm_ft_hit;
int dvm_fuse_targets_reserve_hits(dvm_fuse_targets* h, int max_hits);
int dvm_fuse_targets_run_hits(dvm_fuse_targets* h, const dvm_ft_points* P, const uint8_t* skip, float th,
                              int32_t* hit_off /* [T + 1] */, dvm_ft_hit* hits, int hit_cap, int32_t* n_hits);

/* The BoW searches of LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:722-731): ORBmatcher::SearchByBoW(mpCurrentKF, vpCovKFi[j],
 * vvpMatchedMPs[j]) (ORBmatcher.cc:709-834) once per candidate and covisible keyframe -- up to 11 per candidate, 33 per candidate list --
 * for ALL target keyframes as ONE chain.  The search of one pair walks the vocabulary nodes both FeatureVectors share; a keypoint of the
 * target lies in exactly one node, so the claims of one node (vbMatched2) never reach another, and targets share nothing: every
 * (target, node of cur) pair is an independent sequential walk, one wave each.
 *
 *   one packed upload of cur and all targets (keypoint angles, descriptors, a has-good-map-point flag, the FeatureVectors; every target's
 *   span rounded up), TWO launches -- the search over (target, node) pairs, the rotation check (ComputeThreeMaxima, :813-831) per target --
 *   and ONE copy back behind ONE synchronisation.  The call never allocates after dvm_bow_targets_reserve.
 *
 * Contract: match_idx2[t * cur->n + i] is the keypoint of target t that SearchByBoW(cur, targets[t]) leaves matched to keypoint i of cur
 * (vpMatches12[i] == targets[t]'s map point of that keypoint), -1 where it leaves NULL; nmatches[t] is that call's return value.  Both
 * equal the reference's sequential walk bit for bit, with its acceptance rule best < TH_LOW = 50 (strict, :785) and
 * (float)best < nnratio * (float)second.  Row t does not depend on the other targets.
 *
 * Errors, all reported before anything runs and leaving the handle usable: DVM_ERR_CAPACITY -- cur's keypoints, the targets or their
 * total keypoints beyond the reservation; DVM_ERR_INVALID -- a keyframe with n > 8192, a missing array, node ids not strictly ascending
 * as unsigned, fv_off not non-decreasing from 0, an fv_feat entry outside [0, n), an fv_feat entry listed twice within one keyframe (the
 * independence of the nodes rests on it).  dvm_bow_targets_create returns DVM_ERR_NO_DEVICE without a GPU.  Legal: n_targets = 0 (writes
 * nothing), cur->n = 0 or cur->fv_n = 0 (nmatches all 0), a target with n = 0 or fv_n = 0 (its row is -1, its count 0).
 * sizeof(dvm_bt_keyframe) == 64 (LP64). */
typedef struct {
  int32_t n, fv_n;                  /* keypoints; nodes of mFeatVec */
  const dvm_keypoint* kps;          /* mvKeysUn (the search reads .angle only) */
  const uint8_t* desc;              /* n x 32 */
  const int32_t* mp;                /* n: >= 0 where GetMapPointMatches()[i] != NULL */
  const uint8_t* bad;               /* n: isBad() of that point; may be NULL */
  const int32_t *fv_node, *fv_off, *fv_feat;   /* mFeatVec flattened, nodes ascending as unsigned (dvm_ref_keyframe's convention) */
} dvm_bt_keyframe;
typedef struct dvm_bow_targets dvm_bow_targets;
int dvm_bow_targets_create(int device, dvm_bow_targets** out);
void dvm_bow_targets_destroy(dvm_bow_targets* h);
/* the working set for calls up to these sizes (grow-only; the search never allocates) */
int dvm_bow_targets_reserve(dvm_bow_targets* h, int max_cur_keypoints, int max_targets, int max_total_target_keypoints);
/* match_idx2 [n_targets * cur->n], nmatches [n_targets] */
int dvm_search_by_bow_targets(dvm_bow_targets* h, const dvm_bt_keyframe* cur, int n_targets, const dvm_bt_keyframe* targets, float nnratio,
                              int check_ori, int32_t* match_idx2, int32_t* nmatches);
/* HIP-event timing (measurement only): enable != 0 makes the search record events; ms[2] = search kernel, settle kernel of the last call */
int dvm_bow_targets_profiling(dvm_bow_targets* h, int enable);
int dvm_bow_targets_last_kernel_ms(dvm_bow_targets* h, float* ms);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:384-453), batched: map point p owns the descriptors
 * desc[off[p] .. off[p+1]) (32 B each, its observations in the reference's iteration order); best_idx[p] = index
 * inside that range of the descriptor with the least median Hamming distance to the others (median =
 * sorted_row[0.5 * (N - 1)], first strictly smaller wins), best_median[p] = that median.  Empty range: -1;
 * more than 512 observations: -2 (the caller keeps its CPU path for those).
 * Host pointers (synchronous) or device pointers (asynchronous on `stream`). */
int dvm_distinctive_descriptors(const uint8_t* desc, const int32_t* off, int n_points, int32_t* best_idx, int32_t* best_median,
                                int on_device, void* stream);

/* DBoW2 vocabulary tree on the device + per-feature transform (reference Thirdparty/DBoW2/DBoW2/
 * TemplatedVocabulary.h:1098-1138, FORB::distance FORB.cpp:80-97).  Nodes 0..n_nodes-1, node 0 = root;
 * children[child_off[i] .. child_off[i+1]) in m_nodes[i].children order (empty = leaf); desc 32 B per node; weight and
 * word_id as in m_nodes[i] (word_id < 0 for inner nodes); L = m_L.  dvm_vocab_transform fills, for feature f,
 * word_id / weight of the leaf reached and node_id = the node on the path at level L - levelsup (0 if that level is
 * <= 0; -1 where the reference leaves *nid unset because the leaf lies above that level).  dvm_vocab_create refuses
 * (DVM_ERR_INVALID) lists that are no tree the walk leaves: a child id not above its parent's (nodes are numbered in
 * creation order, as DBoW2 and loadFromTextFile do), a node under two parents or under none.  The BowVector /
 * FeatureVector bookkeeping on top of it is host code (dvm_slam_amd/host/orb_vocabulary.cpp). */
typedef struct dvm_vocab dvm_vocab;
int dvm_vocab_create(int device, int n_nodes, const int32_t* child_off, const int32_t* children, const uint8_t* desc,
                     const double* weight, const int32_t* word_id, int L, dvm_vocab** out);
void dvm_vocab_destroy(dvm_vocab* v);
int dvm_vocab_transform(const dvm_vocab* v, const uint8_t* features, int n, int levelsup, int32_t* word_id, int32_t* node_id,
                        double* weight, int on_device, void* stream);

/* BowVectors of the keyframes of a KeyFrameDatabase on the device + the per-query work of its place-recognition searches
 * (reference src/KeyFrameDatabase.cc:43-70 add / erase, :224-808 DetectCandidates / DetectNBestCandidates /
 * CalculateMergeScore): for every stored keyframe at once, the number of words it shares with the query BowVector
 * (= mnPlaceRecognitionWords after the inverted-file walk), the first shared word (with the insertion order this gives the
 * keyframe's position in lKFsSharingWords) and mpVoc->score(query, keyframe) (L1Scoring, cast to float as the reference
 * stores it).  Word ids ascending (std::map order).  The covisibility accumulation and candidate selection on top are
 * host code (dvm_slam_amd/host/keyframe_database.cpp). */
typedef struct dvm_bowdb dvm_bowdb;
int dvm_bowdb_create(int device, dvm_bowdb** out);
void dvm_bowdb_destroy(dvm_bowdb* db);
/* append a keyframe's BowVector; *slot receives its index (slots are never reused) */
int dvm_bowdb_add(dvm_bowdb* db, const int32_t* word_ids, const double* values, int n, int32_t* slot);
int dvm_bowdb_erase(dvm_bowdb* db, int32_t slot);
int dvm_bowdb_size(const dvm_bowdb* db);   /* slots handed out so far */
/* common[s] = shared words (-1: erased slot), first_word[s] = smallest shared word id (-1 none), score[s]; arrays of
 * dvm_bowdb_size() entries, host pointers, synchronous. */
int dvm_bowdb_query(dvm_bowdb* db, const int32_t* word_ids, const double* values, int n, int32_t* common, int32_t* first_word,
                    float* score);
/* out[4] = {slots ever added, live slots, words stored (live + erased, shrinks when the store is repacked), word capacity}.
 * Erased slots keep their number; their words are reclaimed by a repack once they outnumber the live words. */
int dvm_bowdb_stats(const dvm_bowdb* db, int64_t out[4]);

/* TrackWithMotionModel-style frame-to-frame search over a batch (ORBmatcher.cc:1596-1611, mono):
 * pair i (0 <= i < count) searches train slot first_slot+i for every keypoint of frame i-1 of the
 * device arrays (d_kps + (i-1)*kps_stride, ...); pair 0 takes its queries from the carry frame
 * (d_carry_*, may be NULL: pair 0 then yields 0 matches).  Window th*scale[octave], octaves
 * [o-1,o+1].  d_out + i*out_stride receives `cap` dvm_match per pair, d_nq_out[i] the query count. */
int dvm_match_frames_batch(const dvm_frame* train, int first_slot, int count, const dvm_keypoint* d_kps,
                           int64_t kps_stride, const uint8_t* d_desc, int64_t desc_stride, const int32_t* d_n,
                           const dvm_keypoint* d_carry_kps, const uint8_t* d_carry_desc, const int32_t* d_carry_n,
                           int cap, float th, const float* d_scale_factors, int nlevels, dvm_match* d_out,
                           int64_t out_stride, int32_t* d_nq_out, void* stream);

/* --------------------------------------------------------------------------- bundle adjustment */
/* Optimizer::BundleAdjustment / LocalBundleAdjustment (Optimizer.cc:55-356,1030-1387): SE3 camera
 * vertices (fixed or free), XYZ landmark vertices (all marginalised), one EdgeSE3ProjectXYZ per
 * observation with information I*inv_sigma2 and an optional Huber kernel, solved by g2o's
 * BlockSolver_6_3 + Levenberg recipe in FP64.  Cameras are (tx,ty,tz,qx,qy,qz,qw), world->camera. */
typedef struct { int32_t pose, point; double u, v, inv_sigma2; } dvm_ba_edge;
typedef struct { double fx, fy, cx, cy, huber_delta; /* <= 0: no robust kernel (bRobust=false) */ } dvm_ba_camera;
typedef struct {
  int32_t iterations, total_trials, stop_reason, kernel_us; /* stop: 0 iteration budget / stop flag, 1 LM terminate, 2 Mur-Artal criterion;
                                                          kernel_us: dvm_ba_optimize_windows_fast only -- the launch's duration (HIP events), 0 elsewhere */
  double chi2_initial, chi2_final, lambda_final;
  int32_t trials_per_iter[64];
  double chi2_per_iter[64], lambda_per_iter[64];
  double ms_structure, ms_optimize;                   /* host wall time: graph build / optimize() */
  int32_t spec_trials, spec_kept;                     /* trials whose successor was enqueued on the device's own accept decision,
                                                         and how many of those the host's decision confirmed bit for bit */
} dvm_ba_stats;
typedef struct dvm_ba dvm_ba;
int dvm_ba_create(int device, dvm_ba** out);
void dvm_ba_destroy(dvm_ba* h);
/* builds the graph (vertex order, incidence lists, reduced-camera block pattern) and uploads it */
int dvm_ba_set_problem(dvm_ba* h, const double* poses, const uint8_t* fixed, int P, const double* points, int L,
                       const dvm_ba_edge* edges, int E, const dvm_ba_camera* cam);
/* dvm_ba_set_problem on a camera model (dvm_camera_model above): every EdgeSE3ProjectXYZ of the problem takes its error from
 * obs - pCamera->project(Xc) and its Jacobians from -pCamera->projectJac(Xc) * R and * SE3deriv (OptimizableTypes.h:102,
 * OptimizableTypes.cpp:147-154) of that one camera.  DVM_ERR_INVALID, before anything runs, for a NULL model, a model outside {0, 1} or a
 * zero focal length.  Every call sets the handle's model again; dvm_ba_optimize, dvm_ba_set_edge_flags, dvm_ba_get_result,
 * dvm_ba_edge_chi2 and the measurement aids then work as on any problem.
 *   model 0: forwards to dvm_ba_set_problem with (double)p[0..3] and huber_delta -- everything afterwards is that call's result bit for
 *     bit, the sequential-order form of problems with <= 6 free cameras included.
 *   model 1 (KannalaBrandt8): the residual's theta is the float atan2f(sqrtf((float)(x^2 + y^2)), (float)z) of project(Vector3d), the
 *     Jacobian's the double atan2, as in the reference; a point on the optical axis has a NaN Jacobian, as in the reference.  The tile
 *     solver handles EVERY problem size under this camera, the <= 6 free cameras of a local-BA window too: what the sequential-order
 *     kernels promise is g2o's bits, and the residual is quantised by an atan2f whose last bit no two implementations share, so that
 *     promise does not exist here.  ACCURACY CONTRACT (tests/test_gpu_ba_kb8.py, against the float64 restatement of the recipe in
 *     tests/ba_kb8_scene.py): the LM accept / reject sequence and the stop reason are identical, and poses and landmarks agree within
 *     10 x what the restatement itself moves by when every edge's theta is one float32 ulp off (measured per scene set, docs/NOTEBOOK.md
 *     section 18; never less than 1e-6) -- on scenes whose trial sequence survives that ulp.
 * Pinhole-only as before: dvm_ba_set_problem_sharded, dvm_ba_optimize_windows (the sequential-order form), dvm_ba_optimize_batch.  The
 * cluster form and the pool take a model per window: dvm_ba_optimize_windows_fast_cam, dvm_ba_pool_optimize_cam below. */
int dvm_ba_set_problem_cam(dvm_ba* h, const double* poses, const uint8_t* fixed, int P, const double* points, int L,
                           const dvm_ba_edge* edges, int E, const dvm_camera_model* model, double huber_delta);
/* optimizer.optimize(iterations); stop_flag (may be NULL) is g2o's forceStopFlag: polled between
 * iterations and trials, may be written by another thread (LocalMapping.cc:305,359).
 * ACCURACY CONTRACT (tests/test_gpu_ba_weak.py, tests/test_gpu_config_size.py, tests/test_gpu_ba_window.py), against the CPU
 * restatement of g2o's recipe (oracle/ba_oracle.cpp; the reference itself cannot be run here -- "parity unpinned"):
 *   - problems with <= 6 free cameras run every sum in g2o's own sequential order: BIT-IDENTICAL states, chi2, lambda, trial sequence;
 *   - larger problems are solved with parallel (tile) summation orders: the LM accept / reject sequence is identical and poses and
 *     landmarks agree within 1e-6 -- EXCEPT on weakly constrained problems (two- or three-view landmarks, few hundred points: a gauge
 *     that is barely held), where the result of the recipe itself moves by more than 1e-6 when nothing but the ORDER of the edge list
 *     changes.  The reference adds its edges in heap-address order (std::map<KeyFrame*, ...>, Optimizer.cc:1108-1230), so its own result is
 *     one sample of that spread.  There the bound is 10 x the distance between two runs of the restatement on permuted edge lists,
 *     measured per problem by the test; observed: up to 4e-5 on an 87-keyframe / 273-landmark / 3-view problem whose own spread is 2e-5. */
int dvm_ba_optimize(dvm_ba* h, int iterations, const volatile uint8_t* stop_flag, dvm_ba_stats* stats);
int dvm_ba_get_result(dvm_ba* h, double* poses, double* points);
/* Two-round solves on one graph -- the welding bundle adjustment of a map merge (Optimizer.cc:3474-3519: optimize(5), then
 * e->setLevel(1) on the outliers, e->setRobustKernel(0) on every edge, initializeOptimization(0), optimize(10)) -- without a
 * second dvm_ba_set_problem: flags[e] bit 0 = the edge stays at level 0 (a level-1 edge is outside the active set: it
 * contributes nothing and dvm_ba_edge_chi2 keeps reporting the chi2 of its last evaluation, as g2o's e->chi2() does), bit 1 =
 * the edge keeps its robust kernel (huber_delta of the problem).  Takes effect with the next dvm_ba_optimize, which starts
 * from the estimates the previous one left (iteration 0 again: fresh computeLambdaInit).  NULL: every edge active and
 * robust again.  Not available on a landmark-sharded problem. */
#define DVM_BA_EDGE_ACTIVE 1
#define DVM_BA_EDGE_ROBUST 2
int dvm_ba_set_edge_flags(dvm_ba* h, const uint8_t* flags);
/* BASELINE.json config 5 (global BA sharded over the GPUs of a node; the reference solves it on one CPU thread,
 * Optimizer.cc:44-53 -> block_solver.hpp:381-439): rank r of `world` receives the WHOLE problem (so that the free-camera
 * order, the block pattern and the tile schedule are identical everywhere) but evaluates only the observations of the
 * landmarks it owns (point % world == rank): edge pass, Hll / Hpl, its share of Hpp / b and of the Schur complement.  Per LM
 * trial the partial reduced camera systems -- the structurally non-zero 64x64 tiles, rhs row included -- are summed over the
 * ranks through the caller's all-reduce (RCCL over xGMI), every rank factors the sum redundantly, back-substitutes its own
 * landmarks and moves all cameras; chi2 / scale are two more host scalars.  dvm_ba_optimize ends with one exchange of the
 * landmarks, so dvm_ba_get_result returns the full state on every rank.  dvm_ba_edge_chi2 then covers the LOCAL edges
 * (those with point % world == rank, in input order).
 * dvm_allreduce_fn: in-place reduction over all ranks of n doubles at `buf` -- device memory (on_host = 0; must be ordered
 * after the work already queued on `stream` and before work queued later) or host memory (on_host = 1); op 0 = sum,
 * 1 = max; returns 0 on success.  d_buf: device buffer of at least dvm_ba_allreduce_doubles() doubles owned by the caller
 * (e.g. a torch tensor, so that torch.distributed can reduce it). */
typedef int (*dvm_allreduce_fn)(void* ctx, void* buf, int64_t n, int on_host, int op, void* stream);
int dvm_ba_set_problem_sharded(dvm_ba* h, const double* poses, const uint8_t* fixed, int P, const double* points, int L,
                               const dvm_ba_edge* edges, int E, const dvm_ba_camera* cam, int rank, int world);
int dvm_ba_set_allreduce(dvm_ba* h, dvm_allreduce_fn fn, void* ctx, void* d_buf, int64_t cap_doubles);
int64_t dvm_ba_allreduce_doubles(const dvm_ba* h);
/* Measurement aids (bench.py).  dvm_ba_schedule_info: the symbolic tile factorisation of the current problem,
 * out[12] = {levels launched, tile columns, strips (trsm tiles), update targets, (target, contributor) products, of which on
 * diagonal targets, non-zero tiles, ldS, free cameras, non-zero 6x6 blocks, local edges, tiles per side} -- what the executed
 * FLOP count of one LM trial follows from.  dvm_ba_profile: enable (1) / disable (0) / read only (-1) HIP-event timing of the
 * four phases of a trial; ms4 = {linearise, Schur complement, tile Cholesky + back substitution, landmarks + update + chi2}
 * accumulated since the last enable, over *trials trials / *iters iterations. */
int dvm_ba_schedule_info(const dvm_ba* h, int64_t* out);
/* dvm_ba_solve_info: which form of the reduced solve (the replacement of g2o's LinearSolverEigen::solve,
 * Thirdparty/g2o/g2o/solvers/linear_solver_eigen.h:89-112, under BlockSolver::solve, g2o/core/block_solver.hpp:354-486) the current
 * problem runs: out[6] = {form: 0 = one launch (or two) per elimination-tree level, 1 = the flow form -- the whole factorisation + back
 * substitution as ONE persistent launch of tile tasks, chosen from 5 elimination levels on while the tasks are few per workgroup --, tile tasks of the flow
 * form, chains (= leaves of the elimination tree), workgroups launched, KEPT landmarks, camera tiles}.  The two forms sum in the same order
 * (same numbers).  Kept landmarks: when a few landmarks seen from places far apart on the trajectory are what makes the elimination tree
 * deep (>= 12 levels), up to 210 of them are not eliminated into the Schur complement but stay unknowns of the reduced system, in tiles of
 * their own behind the camera tiles -- the same linear system as g2o's, eliminated in another order (results agree within the 1e-6 of
 * the accuracy contract, not bit for bit).  DVM_BA_BORDER=0 in the environment switches that off. */
int dvm_ba_solve_info(const dvm_ba* h, int64_t* out);
int dvm_ba_profile(dvm_ba* h, int enable, double* ms4, int32_t* trials, int32_t* iters);
/* per-edge chi2() as g2o reports it after optimize(), and isDepthPositive() (outlier tests of
 * Optimizer.cc:1317-1354); either output may be NULL */
int dvm_ba_edge_chi2(dvm_ba* h, double* chi2, uint8_t* depth_positive);
void* dvm_ba_stream(dvm_ba* h);

/* K INDEPENDENT bundle adjustments in one launch: the LocalBundleAdjustment windows (Optimizer.cc:1030-1387) of several agents that
 * share this GPU (BASELINE.json config 4 with more agents than GPUs), or the GlobalBundleAdjustemnt of a freshly initialised
 * two-keyframe map (Tracking.cc:2330, Optimizer.cc:55-356).  Every window is what one dvm_ba_set_problem + dvm_ba_optimize(iterations)
 * + dvm_ba_get_result + dvm_ba_edge_chi2 sequence would be given and return; one workgroup per window runs the whole
 * optimizer.optimize(iterations) on the device.
 * Summation order: every sum of a window runs in the order of g2o's single-threaded code (edges in input order per Hessian block
 * and in chi2, landmarks in index order in the Schur complement, columns in order in the Cholesky factorisation) and sin / cos /
 * pow(x, 3) are the fixed double-precision sequences of csrc/f64_spec.h, so the result is BIT-IDENTICAL to the CPU restatement of
 * g2o's recipe -- which matters for windows with a weak gauge (one or two free cameras), whose result moves by 1e-3 and more when
 * only the order of the floating-point sums changes.
 * Limits: at most 30 free cameras per window (DVM_ERR_CAPACITY above; dvm_ba_optimize has no limit).  Host pointers, synchronous.
 * stop_flag (may be NULL) is polled by the kernel between iterations and trials, for all windows.  stats: K entries or NULL;
 * ms_optimize = wall time of the whole call (upload, launch, download), ms_structure = this window's share of the host set-up. */
typedef struct {
  int32_t n_poses, n_points, n_edges, iterations;
  const double* poses;         /* [n_poses][7]  (tx,ty,tz,qx,qy,qz,qw), world -> camera */
  const uint8_t* fixed;        /* [n_poses] */
  const double* points;        /* [n_points][3] */
  const dvm_ba_edge* edges;    /* [n_edges], pose / point are indices into THIS window's arrays */
  dvm_ba_camera cam;
  double* poses_out;           /* [n_poses][7] or NULL */
  double* points_out;          /* [n_points][3] or NULL */
  double* edge_chi2_out;       /* [n_edges] or NULL: e->chi2() after the last computeActiveErrors */
  uint8_t* depth_positive_out; /* [n_edges] or NULL: isDepthPositive() at the result */
} dvm_ba_window;
int dvm_ba_optimize_windows(int device, const dvm_ba_window* windows, int K, const volatile uint8_t* stop_flag, dvm_ba_stats* stats);
/* The same K windows, ONE launch, the whole Levenberg-Marquardt control on the device -- with every sum as a tree in a FIXED order instead of
 * g2o's sequential one, and a CLUSTER of G workgroups per window (G = the largest of 8 / 4 / 2 / 1 for which the launch's
 * 8 * ceil(K / 8) * G workgroups are resident at once; DVM_BA_CLUSTER forces it): the data-parallel phases are split over the cluster and
 * separated by agent-scope barriers, workgroup 0 solves the reduced system in its LDS.  One window: 2.5 ms (tile solver 1.1 ms, the
 * sequential-order kernel 15 ms); 32 windows: 2.8 ms of kernel, 4.2-4.8 ms per call from host arrays = 67-76 k LM iterations/s; 128 windows: 15-17 ms =
 * 75-84 k.  Deterministic and
 * independent of G and of the other windows of the call; equal to the CPU recipe to the general solver's contract -- same LM trial
 * sequence, poses / landmarks within 1e-6 on well-posed windows -- not bit for bit.  Up to 30 free cameras per window (DVM_ERR_CAPACITY
 * beyond: dvm_ba_optimize_batch).  A barrier that times out (a workgroup of a cluster not resident: other work holds compute units) makes the
 * call repeat the batch with G = 1, which needs no co-residency.  The calling thread keeps its windows' host tables for the next call
 * (~2 MB per window).  This is the call for the LocalBundleAdjustment windows of several agents sharing a GPU (Optimizer.cc:1030-1387,
 * LocalMapping.cc:172). */
int dvm_ba_optimize_windows_fast(int device, const dvm_ba_window* windows, int K, const volatile uint8_t* stop_flag, dvm_ba_stats* stats);
/* The shared form for several agents' LocalMapping threads (as dvm_orb_pool / dvm_pose_pool for the tracking threads): dvm_ba_pool_optimize
 * is dvm_ba_optimize_windows_fast for ONE window -- a blocking call from any number of threads; calls that arrive within `window_us`
 * (< 0: 300) of each other run as ONE launch.  The result of a window does not depend on the batch it rode in: every caller gets the bits
 * of a solo dvm_ba_optimize_windows_fast call.  batch_size (may be NULL): how many windows the call's launch held.  No stop flag. */
typedef struct dvm_ba_pool dvm_ba_pool;
int dvm_ba_pool_create(int device, int max_batch, int window_us, dvm_ba_pool** out);
void dvm_ba_pool_destroy(dvm_ba_pool* pool);
int dvm_ba_pool_optimize(dvm_ba_pool* pool, const dvm_ba_window* w, dvm_ba_stats* stats, int* batch_size);
/* dvm_ba_optimize_windows_fast with a camera model PER WINDOW (dvm_camera_model above; models: K entries): the LocalBundleAdjustment windows
 * of a fleet of fisheye agents -- or of a fleet of both kinds -- in one call.  Every EdgeSE3ProjectXYZ of window k takes its error and its
 * Jacobians from models[k], as under dvm_ba_set_problem_cam.  DVM_ERR_INVALID, before anything runs and before the device is touched, for
 * NULL models, any model outside {0, 1} or a zero focal length anywhere in the array; no output is written then.
 *   model 0: the window is the pinhole window of (double)p[0..3] -- what dvm_ba_optimize_windows_fast returns for it with those four
 *     doubles in cam, BIT FOR BIT, results and LM statistics.
 *   model 1 (KannalaBrandt8): the window's cam.fx, fy, cx, cy are NOT read; cam.huber_delta is.  theta of the residual is the float atan2f
 *     of project(Vector3d), the Jacobian's the double atan2, as in the reference; a point on the optical axis has a NaN Jacobian, as in
 *     the reference.  ACCURACY CONTRACT (tests/test_gpu_ba_window_fast_kb8.py), that of dvm_ba_set_problem_cam: against the float64
 *     restatement of the recipe the LM accept / reject sequence and the stop reason are identical and poses and landmarks agree within 10 x
 *     what the restatement itself moves by when every edge's theta is one float32 ulp off (never less than 1e-6); against the tile solver
 *     (dvm_ba_set_problem_cam + dvm_ba_optimize, the same kb8_project: only the summation order differs) the same sequence, and states as
 *     close as the two pinhole forms are to each other.
 * The windows are grouped by model type; each type present runs as one launch of its instantiation of the kernel, one after the other: a
 * homogeneous fleet is ONE launch, a mixed call two.  G is chosen per launch from that launch's window count; the G = 1 repeat after a barrier
 * time-out applies per launch.  A window's result depends neither on its batch, nor on G, nor on the other model types of the call.
 * Limits as for dvm_ba_optimize_windows_fast: more than 30 free cameras in a window is DVM_ERR_CAPACITY, returned before anything runs -- for a
 * fisheye agent the way out is dvm_ba_set_problem_cam + dvm_ba_optimize (dvm_ba_optimize_batch is pinhole-only).  DVM_BA_SPLIT is NOT honoured
 * by this entry: it is always the one launch per model type.  The sequential-order dvm_ba_optimize_windows stays pinhole-only: its promise
 * is g2o's bits, and that promise does not exist under a float atan2f (see dvm_ba_set_problem_cam).
 * dvm_ba_pool_optimize_cam: dvm_ba_pool_optimize for one window and its model.  Calls of different model types -- and dvm_ba_pool_optimize
 * calls -- that arrive within one commit window ride in the same call; every caller gets the bits of a solo
 * dvm_ba_optimize_windows_fast_cam call.  batch_size: how many windows the call held, over all model types. */
int dvm_ba_optimize_windows_fast_cam(int device, const dvm_ba_window* windows, const dvm_camera_model* models /* [K] */, int K,
                                     const volatile uint8_t* stop_flag, dvm_ba_stats* stats);
int dvm_ba_pool_optimize_cam(dvm_ba_pool* pool, const dvm_ba_window* w, const dvm_camera_model* model, dvm_ba_stats* stats, int* batch_size);
/* The same K independent problems solved CONCURRENTLY on the general solver: up to `threads` (<= 0: 4) host threads of this call each
 * drive one solver handle from a process-wide pool and pull windows from a shared counter, so that the launch chains of different
 * windows interleave on the device (one window alone leaves it mostly idle).  Window k gets exactly what dvm_ba_set_problem +
 * dvm_ba_optimize(iterations) + dvm_ba_get_result + dvm_ba_edge_chi2 on a handle of its own give -- no limit on the number of free
 * cameras, parity with the CPU recipe as for dvm_ba_optimize (windows of at most 6 free cameras take the sequential-order kernel
 * there and are bit-identical).  This is the call for several agents' LocalBundleAdjustment windows per GPU
 * (Optimizer.cc:1030-1387, one LocalMapping thread per agent in the reference).  stats: K entries or NULL. */
int dvm_ba_optimize_batch(int device, const dvm_ba_window* windows, int K, int threads, const volatile uint8_t* stop_flag,
                          dvm_ba_stats* stats);
/* csrc/f64_spec.h evaluated on the device for n arguments: out = [sin(x) | cos(x) | x^3], 3 n doubles.  A test aid: the host build of
 * the spec, the device build and the oracle's restatement must agree bit for bit (tests/test_f64_spec.py, tests/test_gpu_ba_window.py). */
int dvm_f64_spec_eval(int device, const double* x, int n, double* out);

/* Optimizer::PoseOptimization (Optimizer.cc:744-1028, monocular edges): `batch` independent frames.
 * Frame f: pose (tx,ty,tz,qx,qy,qz,qw) at pose_in + 7f; n[f] 2D-3D matches stored with a common
 * `stride` (Xw [batch][stride][3], obs [batch][stride][2] = undistorted keypoint, inv_sigma2
 * [batch][stride] = mvInvLevelSigma2[octave]).  Outputs: optimised pose, mvbOutlier flags, and the
 * reference's return value nInitialCorrespondences - nBad.  Host pointers, synchronous; each frame is
 * one workgroup running the 4 x optimize(10) Levenberg rounds entirely on the device. */
int dvm_pose_optimize(int device, const double* pose_in, const double* Xw, const double* obs, const double* inv_sigma2,
                      const int32_t* n, int stride, int batch, const dvm_ba_camera* cam, double* pose_out,
                      uint8_t* outlier, int32_t* n_inliers);
/* The same on a camera model: the edge's error is obs - pCamera->project(Xc) and its Jacobian -pCamera->projectJac(Xc) * SE3deriv
 * (OptimizableTypes.cpp:51-63) of `model`; LM control, rounds, classification and outputs as above.  Model 0 runs the pinhole kernel on
 * (double)p[0..3] and returns what dvm_pose_optimize returns for those doubles, bit for bit.  KannalaBrandt8: the projection takes theta
 * from the FLOAT atan2f, as the reference's Vector3d overload does (KannalaBrandt8.cpp:48-66), so the residual is quantised in theta and
 * poses agree with a host evaluation to about 1e-5 (9.6e-6 measured, tests allow 9.6e-5), not to the 1e-6 of the pinhole kernel; a correspondence on the optical axis has a NaN Jacobian.  The kernel
 * keeps up to 1 280 correspondences per frame (256 x 5) in registers for either model and re-reads the rest from memory every iteration. */
int dvm_pose_optimize_cam(int device, const double* pose_in, const double* Xw, const double* obs, const double* inv_sigma2,
                          const int32_t* n, int stride, int batch, const dvm_camera_model* model, double* pose_out,
                          uint8_t* outlier, int32_t* n_inliers);

/* The shared form for several agents on one GPU (as dvm_orb_pool for the extractor): dvm_pose_pool_optimize is dvm_pose_optimize for ONE
 * frame -- same arguments, same results bit for bit --, callable from any number of threads; calls that arrive within `window_us` of each
 * other and share the camera run as ONE launch of the batched kernel (a workgroup per frame).  A frame with more than 1 280
 * correspondences is handed to dvm_pose_optimize directly.  batch_size (may be NULL): how many frames the call's launch held. */
typedef struct dvm_pose_pool dvm_pose_pool;
int dvm_pose_pool_create(int device, int max_batch, int window_us, dvm_pose_pool** out);
void dvm_pose_pool_destroy(dvm_pose_pool* pool);
int dvm_pose_pool_optimize(dvm_pose_pool* pool, const double* pose_in, const double* Xw, const double* obs, const double* inv_sigma2, int n,
                           const dvm_ba_camera* cam, double* pose_out, uint8_t* outlier, int32_t* n_inliers, int* batch_size);

/* ---- The tracking step of one frame as ONE device chain (csrc/track.cpp): Frame::Frame -> ExtractORB (src/Frame.cc:371-411), then
 * Tracking::TrackWithMotionModel (src/Tracking.cc:2584-2667) = SearchByProjection(CurrentFrame, LastFrame) (src/ORBmatcher.cc:1553-1748)
 * -> Optimizer::PoseOptimization (src/Optimizer.cc:744-1028) -> outlier matches dropped (:2636-2660).
 *   dvm_track_begin   queues the extraction of the frame on the extractor's stream and returns;
 *   dvm_track_finish  queues [Frame::UndistortKeyPoints] -> AssignFeaturesToGrid -> the ranked window search of the caller's projection
 *                     queries -> claim replay + rotation histogram -> PoseOptimization -> outlier flags behind it, synchronises once and
 *                     returns the frame's keypoints / descriptors (what dvm_orb_extract returns) together with the tracking results.
 * The queries are what the loop header of ORBmatcher.cc:1573-1611 produces from LastFrame's map points and the predicted pose (the
 * host library's dvmh_track_with_motion_model builds them while the extraction runs).  CurrentFrame.mvpMapPoints is taken as cleared
 * (Tracking.cc:2603).  Results equal dvm_orb_extract + dvmh_search_by_projection_frames + dvm_pose_optimize bit for bit. */
typedef struct dvm_tracker dvm_tracker;
typedef struct {
  int32_t nq;
  const uint8_t* qdesc;            /* [nq][32] the map points' descriptors */
  const float *qx, *qy, *qr;       /* projection (u, v) and window radius th * mvScaleFactors[nLastOctave] */
  const int32_t *qmin, *qmax;      /* nLastOctave - 1, nLastOctave + 1 */
  const uint8_t* q_claims;         /* [nq] the map point has Observations() > 0 */
  const float* q_angle;            /* [nq] LastFrame.mvKeysUn[i].angle */
  const float* q_pos;              /* [nq][3] GetWorldPos() */
  float bounds[4];                 /* mnMinX mnMaxX mnMinY mnMaxY */
  const dvm_distortion* dist;      /* NULL or k1 == 0: mvKeysUn = mvKeys */
  const float* inv_level_sigma2;   /* mvInvLevelSigma2, nlevels entries */
  int32_t nlevels;
  dvm_ba_camera cam;               /* fx fy cx cy of PoseOptimization's edges */
  double pose_in[7];               /* the predicted Tcw (tx ty tz qx qy qz qw): mVelocity * mLastFrame.GetPose() */
  int32_t th_high, check_ori;      /* ORBmatcher::TH_HIGH (100), mbCheckOrientation */
  int32_t min_matches;             /* 20 (Tracking.cc:2616) */
} dvm_track_queries;
enum { DVM_TRACK_COMPLETE = 0, DVM_TRACK_FEW_MATCHES = 1, DVM_TRACK_REPLAY_ON_HOST = 2, DVM_TRACK_FEW_MAP_MATCHES = 3 };
typedef struct {
  int32_t n, mono_index;           /* the extraction's keypoint count and monoIndex */
  int32_t status;                  /* DVM_TRACK_COMPLETE; FEW_MATCHES: nmatches < min_matches, no pose (search again with the doubled window:
                                      dvm_track_finish with the wider queries); REPLAY_ON_HOST: kept for callers of older builds -- the device now
                                      searches such a query's window again itself (n_requeried), the status is no longer produced */
  int32_t nmatches;                /* SearchByProjection's return value */
  int32_t nmatches_before_rotation;
  int32_t n_edges, n_inliers;      /* PoseOptimization: nInitialCorrespondences and its return value */
  int32_t nmatches_map, nmatches_after;   /* Tracking.cc:2636-2660: nmatchesMap and nmatches after the outliers were dropped */
  int32_t n_requeried;             /* queries whose four ranked candidates were all taken by earlier queries: their windows were searched
                                      again on the device at their turn (ORBmatcher.cc:1613-1650 skips taken keypoints) */
  double pose[7];                  /* the optimised Tcw */
} dvm_track_result;
int dvm_tracker_create(int device, int max_keypoints, int max_queries, dvm_tracker** out);
/* The same for up to max_frames frames per call -- the frames of several agents sharing the GPU at one camera tick: ONE chain of batched
 * launches (extraction of the batch, max_frames grids, ranked searches, claim replays and PoseOptimizations side by side, a workgroup per
 * frame) behind ONE synchronisation.  The extractor handle needs max_batch >= count.  The frames of a call share camera, image bounds,
 * level table and matcher thresholds, and are not undistorted here (k1 != 0: the single-frame call).  Frame b's results equal
 * dvm_track_begin / dvm_track_finish on that frame alone, bit for bit. */
typedef struct {
  dvm_keypoint* kps; uint8_t* desc; int32_t cap;   /* [cap] the extraction (as dvm_orb_extract) */
  dvm_keypoint* kps_un;                            /* [cap] or NULL: mvKeysUn */
  int32_t* assign; uint8_t* outlier;               /* [cap] as dvm_track_finish */
  uint32_t* ranked;                                /* NULL, or [nq][4] (REPLAY_ON_HOST only) */
} dvm_track_frame_out;
int dvm_tracker_create_batch(int device, int max_frames, int max_keypoints, int max_queries, dvm_tracker** out);
/* The camera of the agent this tracker serves (dvm_camera_model above), for every chain of the tracker: dvm_track_finish[_batch],
 * dvm_track_local_map[_batch] and dvm_track_reference_keyframe[_batch], forms (a) and (b).  NULL or model 0 -- what a fresh tracker has --
 * leaves every chain on the cam field of dvm_track_queries / dvm_track_refkf_params, as before.  Model 1 (KannalaBrandt8): isInFrustum's
 * mpCamera->project and PoseOptimization's edges are evaluated on model->p (csrc/camera_model.h) and the structs' cam fields are not read;
 * the frames of a batch share the model.  Such a frame has mvKeysUn = mvKeys and a zero mDistCoef: dist with k1 != 0 is then
 * DVM_ERR_INVALID from dvm_track_finish and from form (a) of dvm_track_reference_keyframe, before anything is queued (the begin stays
 * valid for a corrected call).  The caller's queries (qx, qy) are projections through the same model (dvmh_track_with_motion_model_cam
 * builds them so).  An unknown model or a zero focal length: DVM_ERR_INVALID, the tracker keeps the model it had.  May be called at any
 * time; what a begin or finish prepared before the call is dropped (the second half then returns DVM_ERR_STATE until the next finish): the
 * second half always runs on the model of the finish that prepared it.  Out of scope: a model per frame of a batch, the stereo /
 * two-camera fisheye rigs of the reference (its Nleft branches). */
int dvm_tracker_set_camera_model(dvm_tracker* t, const dvm_camera_model* model);
int dvm_track_begin_batch(dvm_tracker* t, dvm_orb* h, const uint8_t* imgs, int count, int rows, int cols, int stride, int64_t frame_stride, int lap0, int lap1);
/* the same for `count` frames the caller has written into the extractor's page-locked input buffer (dvm_orb_staging): no host copy */
int dvm_track_begin_staged(dvm_tracker* t, dvm_orb* h, int count, int rows, int cols, int lap0, int lap1);
void dvm_tracker_destroy(dvm_tracker* t);
int dvm_track_begin(dvm_tracker* t, dvm_orb* h, const uint8_t* img, int rows, int cols, int stride, int lap0, int lap1);
/* kps / desc [cap]: the extraction; kps_un (may be NULL): mvKeysUn; assign [cap]: per keypoint the index of the query matched to it or -1
 * (BEFORE the outlier drop); outlier [cap]: mvbOutlier as PoseOptimization leaves it (the matches Tracking then drops); ranked (may be
 * NULL): [nq][4] candidate lists, filled for REPLAY_ON_HOST only.  May be called again after one dvm_track_begin (wider window). */
int dvm_track_finish(dvm_tracker* t, dvm_orb* h, const dvm_track_queries* q, dvm_keypoint* kps, uint8_t* desc, int cap, dvm_keypoint* kps_un,
                     int32_t* assign, uint8_t* outlier, uint32_t* ranked, dvm_track_result* res);
/* qs / outs / res: `count` entries, frame b of the dvm_track_begin_batch call.  A frame with fewer than min_matches matches reports
 * DVM_TRACK_FEW_MATCHES; the call may be repeated (all frames, the wider queries for those) after one begin. */
int dvm_track_finish_batch(dvm_tracker* t, dvm_orb* h, int count, const dvm_track_queries* qs, const dvm_track_frame_out* outs, dvm_track_result* res);

/* ---- The second half of the tracked frame, Tracking::TrackLocalMap (src/Tracking.cc:2668-2740), as ONE device chain behind the first:
 * SearchLocalPoints (:3041-3106: the frame's bad points cleared, Frame::isInFrustum(pMP, 0.5) over the local map, the points the frame
 * holds skipped) -> ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (src/ORBmatcher.cc:44-205, mono: ratio
 * 0.8 when best and second share a level, TH_HIGH, no rotation check) -> Optimizer::PoseOptimization (src/Optimizer.cc:744-1028) seeded
 * from the first half's float pose -> mnMatchesInliers (mbOnlyTracking = false).  It runs on the frame's grid and mvKeysUn the first half
 * left on the device (no re-upload of the frame); the table goes up in one asynchronous copy; one synchronisation at the end.
 * UpdateLocalMap (which points form the table) stays with the caller.  Results equal dvm_is_in_frustum + dvmh_search_by_projection_points
 * + dvm_pose_optimize composed in that order, bit for bit. */
typedef struct {
  float pos[3];                    /* GetWorldPos() */
  float normal[3];                 /* GetNormal() */
  float min_dist, max_dist;        /* mfMinDistance, mfMaxDistance as dvm_is_in_frustum takes them (GetMin/MaxDistanceInvariance() are
                                      0.8 / 1.2 times these; PredictScale needs mfMaxDistance itself) */
  uint8_t desc[32];                /* GetDescriptor() */
  int32_t n_obs;                   /* Observations() */
  int32_t bad;                     /* isBad() */
} dvm_local_point;                 /* 72 bytes, one record per mvpLocalMapPoints entry */
typedef struct {
  int32_t n_to_match;              /* nToMatch of SearchLocalPoints (Tracking.cc:3073): in view, not bad, not held by the frame */
  int32_t nmatches;                /* SearchByProjection's return value: every match event */
  int32_t n_requeried;             /* queries whose window the device searched again (fewer than two of four ranked candidates free) */
  int32_t n_cleared_bad;           /* frame points found bad and cleared (Tracking.cc:3047-3049) */
  int32_t n_edges;                 /* PoseOptimization's nInitialCorrespondences */
  int32_t n_inliers;               /* PoseOptimization's return value (0 below 3 edges: the pose is left as it was) */
  int32_t matches_inliers;         /* mnMatchesInliers (mbOnlyTracking = false) */
  int32_t reserved;
  double pose[7];                  /* the optimised Tcw (tx ty tz qx qy qz qw) */
  dvm_se3f Tcw;                    /* the same as the frame stores it (Optimizer.cc:1023-1025) */
  int32_t reserved2;
} dvm_track_local_result;          /* 120 bytes */
/* Allocates the second half's working set for tables of up to max_points entries (at least 16 384 supported; no growth in the hot path).
 * On a tracker of dvm_tracker_create_batch(max_frames = B), max_points is the TOTAL of one dvm_track_local_map_batch call: the sum over
 * its frames of n_b, each rounded up to 64 (at least B x 16 384 supported); the per-keypoint arrays are reserved for B frames.
 * DVM_ERR_CAPACITY for what it cannot hold.  Called again, it replaces the working set; dvm_tracker_destroy frees it. */
int dvm_tracker_reserve_local_map(dvm_tracker* t, int max_points);
/* Right after a dvm_track_finish of ONE frame that returned DVM_TRACK_COMPLETE, on the same tracker and extractor, before the next begin
 * (otherwise DVM_ERR_STATE); once per finish.  pts [n]: the local map (n <= the reservation, else DVM_ERR_CAPACITY); frame_mp [N] (N = the
 * frame's keypoint count): the index into pts of the map point keypoint j holds after the first half, or -1 (every point the frame holds
 * is in the table).  Outputs: mp_out [N] mvpMapPoints after the search (before any outlier drop: monocular TrackLocalMap keeps them);
 * outlier [N] mvbOutlier of the second PoseOptimization (0 where no map point); track_pts (may be NULL) [n]: Frame::isInFrustum's mTrack*
 * fields per entry, in_view = mbTrackInView after SearchLocalPoints (0 for bad entries and those the frame holds). */
int dvm_track_local_map(dvm_tracker* t, dvm_orb* h, const dvm_local_point* pts, int n, const int32_t* frame_mp, float th, int far_points,
                        float th_far, int32_t* mp_out, uint8_t* outlier, dvm_track_point* track_pts /* may be NULL */, dvm_track_local_result* res);
/* The same for the `count` frames of a dvm_track_finish_batch (or a dvm_track_finish: count = 1) -- several agents' frames of one camera
 * tick: ONE upload of all tables, ONE chain of batched launches on the finish's grids, ONE synchronisation.  Accepted right after that
 * finish on the same tracker and extractor with the finish's count, before the next begin, once per finish (otherwise DVM_ERR_STATE);
 * where the finish ran twice (the wider window), the last one counts.  in / out / res / status: `count` entries.
 *   frame b with first-half status DVM_TRACK_COMPLETE: res[b] and out[b] are exactly what dvm_track_local_map gives on that frame alone;
 *     status[b] = DVM_TRACK_COMPLETE.  Its table size n_b may be 0 and differs per frame, as do th, far_points and th_far (th = 5 after a
 *     relocalisation, 15 when lost: Tracking.cc:3083-3106).
 *   any other frame b: skipped -- status[b] = the first half's status, res[b] zeroed, out[b] not written, in[b] not read.
 * frame_mp entries outside [-1, n_b): DVM_ERR_INVALID; the tables' total (each n_b rounded up to 64) beyond the reservation:
 * DVM_ERR_CAPACITY.  DVM_TRACK_BATCH_TIMING=1 prints the call's host phases on stderr. */
typedef struct {
  const dvm_local_point* pts; int32_t n;          /* this agent's mvpLocalMapPoints; n may be 0 */
  const int32_t* frame_mp;                        /* [N_b] index into pts of the point keypoint j holds after the first half, or -1 */
  float th; int32_t far_points; float th_far;     /* SearchByProjection's th (1 / 5 / 15 ...), mbFarPoints, mThFarPoints */
} dvm_local_map_in;                               /* 40 bytes */
typedef struct {
  int32_t* mp_out; uint8_t* outlier;              /* [N_b] as dvm_track_local_map */
  dvm_track_point* track_pts;                     /* [n_b] or NULL */
} dvm_local_map_out;                              /* 24 bytes */
int dvm_track_local_map_batch(dvm_tracker* t, dvm_orb* h, int count, const dvm_local_map_in* in, const dvm_local_map_out* out,
                              dvm_track_local_result* res, int32_t* status);

/* ---- An agent's map points resident on the device (csrc/map_store.cpp).  A map point is written rarely (LocalMapping after a local BA,
 * a fuse or a culling step, under Map::mMutexMapUpdate) and read at camera rate by every frame that sees it: the store keeps the records
 * in device memory, and the two halves of the tracked frame read them by slot (dvm_track_finish_batch_resident,
 * dvm_track_local_map_batch_resident below) instead of carrying them up on every tick.
 *   capacity  fixed at create: slots 0 .. capacity - 1, one dvm_local_point (72 B) each, device addresses stable, no growth
 *             (DVM_ERR_INVALID for capacity < 1, DVM_ERR_CAPACITY when the memory cannot be had).
 *   update    records[k] is written to slot slots[k].  Checked on the host before anything is queued: a NULL argument, a slot outside
 *             [0, capacity) or a slot named twice in the call is DVM_ERR_INVALID and nothing is written.  The records are staged in
 *             page-locked memory and scattered by a kernel on the STORE'S OWN STREAM; the call may return before the kernel has run.
 *             Ordering is by events: every later call that reads the store makes its stream wait for the store's last update, and an
 *             update waits for the last kernel that was queued to read the store -- it never overtakes a chain call in flight.  A second
 *             update waits on the host until the first has left the staging block.
 *   read      slots back, in the order asked (a slot may repeat); synchronous.  Tests and debugging.
 *   Every call that names a slot never written (read, and the chain calls below) is DVM_ERR_INVALID, checked on the host against a
 *   per-slot written flag before anything is queued: no kernel indexes a store with a value the host has not checked.
 * Calls on ONE store -- update, read, and the chain calls that name it -- are not concurrent (the reference holds mMutexMapUpdate around
 * the same writes); different stores are independent. */
typedef struct dvm_map_store dvm_map_store;
int dvm_map_store_create(int device, int capacity, dvm_map_store** out);
void dvm_map_store_destroy(dvm_map_store* s);
int dvm_map_store_capacity(const dvm_map_store* s);
int dvm_map_store_update(dvm_map_store* s, int n, const int32_t* slots, const dvm_local_point* records);
int dvm_map_store_read(dvm_map_store* s, int n, const int32_t* slots, dvm_local_point* out);

/* ---- A map point's record made where it lies: MapPoint::ComputeDistinctiveDescriptors() + MapPoint::UpdateNormalAndDepth() (src/MapPoint.cc:
 * 384-453, 473-540) -- what LocalMapping runs in ProcessNewKeyFrame, at the end of CreateNewMapPoints and at the end of SearchInNeighbors --
 * from the descriptor rows the keyframe slots hold (dvm_keyframe_store, below) and the position the map slot holds.  The call names slots:
 * 8 B per observation and about 25 B per point travel up, 4 B per point come down (which observation's descriptor won, so that the host
 * MapPoint copies its own row).  No camera model is read.  N = a point's observation count, its list in GetObservations() order.
 *   DESCRIPTOR  candidates: the observations on keyframes without DVM_MPR_KF_BAD, in list order (:406).  Winner and median are
 *               dvm_distinctive_descriptors' on that set (median = sorted_row[(N' - 1) >> 1], self distance included, the first strictly
 *               smaller median wins); best_obs_out = the winner's index in the point's FULL list, the record's desc = that keyframe
 *               slot's row.  No candidate: best_obs_out = best_median_out = -1 and desc is not touched (a new point's desc: zeros).
 *   GEOMETRY    (N >= 1) pos = the record's own, or new_pos for a new point.  All N observations count, bad keyframes too (:493-512):
 *               normal = (((0 + t0) + t1) + ...) / (float)N, t = d / |d| per component, d = pos - ow, |d| = sqrt(d0 d0 + (d1 d1 + d2 d2));
 *               max_dist = |pos - ow_ref| * sf_ref[octave of the ref keypoint], min_dist = max_dist / sf_ref[n_levels_ref - 1], the level
 *               table read from the ref keyframe's slot.  float32, one rounding per operation: the bits dvm_ba_resident_commit writes.
 *   the record  n_obs = N in every case.  Old point: pos and bad are kept, only the groups in `what` are written; N = 0: nothing but n_obs.
 *               New point (is_new[p] != 0): the whole record -- pos = new_pos, bad = 0 --; it needs what = both and N >= 1, and its slot
 *               counts as written from this call on.
 *   outputs     best_obs_out -1 where the descriptor was not asked for or not written; geometry_out: pos, normal, min_dist, max_dist as
 *               the record holds them after the call.
 *   refusals    decided on the host before anything is queued: nothing is written, a new slot stays unwritten, dvm_last_error names the
 *               point or keyframe.  DVM_ERR_INVALID: a NULL required array (ref_obs is required with GEOMETRY, is_new and new_pos come
 *               together); what = 0 or unknown bits; stores on different devices; obs_off not monotone from 0 to n_obs; a map slot outside
 *               the store or named twice; an old point's slot never written; a new point with N = 0 or what != both; obs.kf outside
 *               [0, n_kfs); a keyframe slot outside its store, never written or removed; unknown keyframe flags; kp outside [0, n) of its
 *               slot; ref_obs outside [0, N) when GEOMETRY and N >= 1.  An entry with DVM_MPR_KF_BAD may carry slot = -1 (the keyframe
 *               has left the store): the kp of its observations is then not checked, and it may not be a point's ref (DVM_ERR_INVALID).
 *               DVM_ERR_CAPACITY: a point with more than 512 observations.
 *   ordering    the inputs go up in one copy on the calling thread's staging stream; ONE launch (k_mp_refresh, a wavefront per point)
 *               there.  The call is a WRITER of the map store -- it waits for the last kernel queued to read it and for the last update or
 *               commit -- and a READER of the keyframe store (it waits for the last put; the next put waits for it).  It synchronises
 *               once; the outputs are valid and new slots are written when it returns.
 *   last_refresh_bytes   what the last refresh sent up (its one copy) and what came down (the kernel's writes into page-locked memory).
 *   profile / last_refresh_ms   with profiling enabled, k_mp_refresh's time by HIP events (measurement only).
 * sizeof(dvm_mp_obs) == 8 (kf 0, kp 4); sizeof(dvm_mp_refresh_kf) == 20 (slot 0, flags 4, ow 8); sizeof(dvm_mp_refresh) == 96 (LP64:
 * n_points 0, n_kfs 4, n_obs 8, what 12, mp_slot 16, obs_off 24, obs 32, ref_obs 40, kfs 48, is_new 56, new_pos 64, best_obs_out 72,
 * best_median_out 80, geometry_out 88). */
typedef struct { int32_t kf, kp; } dvm_mp_obs;                     /* 8 B: index into the call's keyframe table; keypoint index in that keyframe */
#define DVM_MPR_KF_BAD 1u
typedef struct { int32_t slot; uint32_t flags; float ow[3]; } dvm_mp_refresh_kf;   /* 20 B: keyframe-store slot, pKF->isBad(), GetCameraCenter() */
#define DVM_MPR_DESCRIPTOR 1u
#define DVM_MPR_GEOMETRY   2u
typedef struct {
  int32_t n_points, n_kfs, n_obs; uint32_t what;   /* what: DESCRIPTOR, GEOMETRY or both */
  const int32_t* mp_slot;          /* [n_points] map-store slot of each point */
  const int32_t* obs_off;          /* [n_points + 1] CSR, 0 .. n_obs */
  const dvm_mp_obs* obs;           /* [n_obs] a point's observations in MapPoint::GetObservations() order */
  const int32_t* ref_obs;          /* [n_points] index INSIDE the point's own list of mpRefKF's observation */
  const dvm_mp_refresh_kf* kfs;    /* [n_kfs] */
  const uint8_t* is_new;           /* [n_points] or NULL (none new) */
  const float* new_pos;            /* [n_points][3] GetWorldPos() of the new points (rows of old points not read); NULL iff is_new is NULL */
  int32_t* best_obs_out;           /* [n_points] index inside the point's list of the winning observation; -1: descriptor not written */
  int32_t* best_median_out;        /* [n_points] or NULL */
  float* geometry_out;             /* [n_points][8] pos, normal, min_dist, max_dist as written, or NULL */
} dvm_mp_refresh;
struct dvm_keyframe_store;
int dvm_map_store_refresh(dvm_map_store* ms, const struct dvm_keyframe_store* ks, const dvm_mp_refresh* in);
int dvm_map_store_last_refresh_bytes(const dvm_map_store* ms, int64_t* host_to_device, int64_t* device_to_host);
int dvm_map_store_profile(dvm_map_store* ms, int enable);
int dvm_map_store_last_refresh_ms(const dvm_map_store* ms, float* kernel_ms);

/* ---- An agent's keyframes resident on the device (csrc/keyframe_store.cpp): the keyframe-side counterpart of dvm_map_store.  What a
 * KeyFrame holds once ComputeBoW has run never changes -- mvKeysUn, mDescriptors, the level tables, the image bounds, mFeatVec and the
 * feature grid --, LocalMapping names the same neighbours step after step and LoopClosing::SearchAndFuse the same hundred keyframes: the
 * store keeps them, grid included, in device memory, and the LocalMapping chains read them by slot (dvm_fuse_targets_set_resident,
 * dvm_create_new_map_points_resident below) instead of carrying 60 - 70 B per keypoint up and rebuilding every grid on every call.
 * The pose and mvpMapPoints change between two LocalMapping steps and stay per-call arguments.
 *   create    `capacity` slots of fixed size for up to `slot_keypoints` keypoints each (1 .. 8192), ONE device block that never moves:
 *             a slot's device addresses are stable.  A slot holds the arrays as put, the three level tables, the FeatureVector and the
 *             keyframe's grid (the layout: csrc/kf_store_layout.h).  DVM_ERR_INVALID for capacity < 1 or slot_keypoints outside
 *             [1, 8192], DVM_ERR_CAPACITY when the memory cannot be had, DVM_ERR_NO_DEVICE without a GPU.
 *   put       kfs[k] goes to slot slots[k].  Checked on the host before anything is queued, each failure naming the keyframe, nothing
 *             written: DVM_ERR_CAPACITY -- n or fv_n beyond slot_keypoints; DVM_ERR_INVALID -- a slot outside [0, capacity) or named
 *             twice in the call, n < 0, n_levels outside [1, 64], a keypoint's octave outside the level tables, empty image bounds,
 *             fv_off not monotone from 0, more features than keypoints, a feature outside [0, n), nodes not ascending as unsigned, a
 *             missing array (the three level tables are all required).  The batch is packed into a page-locked staging block, sent
 *             with ONE copy and moved by ONE launch -- k_kfs_put, one 1 024-thread workgroup per keyframe, which also builds the grid
 *             in the slot with the function dvm_frame_build and dvm_fuse_targets_set run, so a resident grid has the order a per-call
 *             set produces.  On the STORE'S OWN STREAM; put does not wait.  A batch larger than the staging block goes in rounds.
 *   remove    the slots are empty again (host state; with rows set -- below -- also the slots' row lengths, queued as a put).  A slot
 *             outside [0, capacity) or not written: DVM_ERR_INVALID, nothing changed.
 *   Ordering is dvm_map_store's: every chain call that reads the store makes its stream wait for the store's last put, and a put
 *   waits for the last kernel queued to read the store -- it never overtakes a reader in flight.
 *   Every slot carries a written flag and a generation counter (put and remove bump it).  A chain call that names a slot never
 *   written, or removed, is DVM_ERR_INVALID, checked on the host before anything is queued.
 *   debug_read  one slot back, synchronous (tests): the counts and scalars always, every array whose pointer is not NULL -- kps, desc
 *             [n], fv_node [fv_n], fv_off [fv_n + 1, when fv_n > 0], fv_feat [n_feat], the level tables [n_levels], the grid: skp [n_sorted][4]
 *             (x, y, octave bits, cell bits), sidx [n_sorted], sdesc [n_sorted][32], cell_start [3076].  Buffers sized for slot_keypoints
 *             (64 for the tables) hold any slot.
 * Calls on ONE store are not concurrent; a store outlives every chain handle set on it.  sizeof(dvm_kfs_keyframe) == 120,
 * sizeof(dvm_kfs_readback) == 160 (LP64). */
typedef struct {                       /* what is immutable in a KeyFrame once ComputeBoW has run */
  int32_t n;
  const dvm_keypoint* kps;             /* mvKeysUn */
  const uint8_t* desc;                 /* mDescriptors, n x 32 */
  int32_t fv_n;                        /* mFeatVec, dvm_np_keyframe's convention; fv_n = 0 is legal */
  const int32_t *fv_node, *fv_off, *fv_feat;
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y;
  const float *scale_factors, *level_sigma2, *inv_level_sigma2;   /* [n_levels] each */
  float log_scale_factor;
  int32_t n_levels;
} dvm_kfs_keyframe;
typedef struct {
  int32_t n, fv_n, n_feat, n_levels, n_sorted, n_total;
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y, log_scale_factor;
  uint32_t generation;
  dvm_keypoint* kps;
  uint8_t* desc;
  int32_t *fv_node, *fv_off, *fv_feat;
  float *scale_factors, *level_sigma2, *inv_level_sigma2;
  float* skp;
  int32_t* sidx;
  uint8_t* sdesc;
  int32_t* cell_start;
} dvm_kfs_readback;
typedef struct dvm_keyframe_store dvm_keyframe_store;
int dvm_keyframe_store_create(int device, int capacity, int slot_keypoints, dvm_keyframe_store** out);
void dvm_keyframe_store_destroy(dvm_keyframe_store* s);
int dvm_keyframe_store_capacity(const dvm_keyframe_store* s);
int dvm_keyframe_store_slot_keypoints(const dvm_keyframe_store* s);
int dvm_keyframe_store_put(dvm_keyframe_store* s, int n, const int32_t* slots, const dvm_kfs_keyframe* kfs);
int dvm_keyframe_store_remove(dvm_keyframe_store* s, int n, const int32_t* slots);
int dvm_keyframe_store_debug_read(dvm_keyframe_store* s, int slot, dvm_kfs_readback* out);

/* ---- A put straight from device memory: when Tracking::CreateNewKeyFrame promotes the current frame, its mvKeysUn and descriptors lie
 * in device memory (the extractor's result, the tracker's frame after a finish) and KeyFrame::ComputeBoW is device code.
 * dvm_keyframe_store_put_device computes the BowVector and the FeatureVector on the device and fills the slot there; per keyframe the
 * item record and the three level tables travel up (832 B, nothing per keypoint), the BowVector and the FeatureVector come down
 * (KeyFrameDatabase::add and the host mirrors need them).
 *   put_device  kfs[k] goes to slot slots[k].  The outcome equals dvm_keyframe_store_put of the same keyframe with fv_* set to what
 *             dvmh_vocab_transform(features = desc, levelsup) returns: every array dvm_keyframe_store_debug_read returns is equal bit
 *             for bit, and the slot serves every resident chain (a feature lies in ONE node by construction).  `stream` is the stream
 *             that produced the arrays (NULL: the null stream); the work is ordered behind it by an event and runs on the STORE'S OWN
 *             STREAM under the store's ordering rule (it waits for the last reader, readers wait for it).  Four kinds of launches:
 *             k_kfs_dev_check (the count and the octaves of every keyframe of the call), k_vocab_transform per keyframe,
 *             k_kfs_dev_bow (ComputeBoW's bookkeeping, the FeatureVector into the slot), k_kfs_dev_put (keypoints, descriptors,
 *             tables, the grid).  Unlike put the call synchronises, ONCE: the host's slot record and `outs` are read from mapped
 *             memory after that wait.  Checked on the host before anything is queued, each naming the keyframe: DVM_ERR_INVALID --
 *             a slot outside [0, capacity) or named twice, n < 0, a NULL or not 4-byte-aligned array with n > 0, n_levels outside
 *             [1, 64], empty bounds, a missing table, a vocabulary on another device; DVM_ERR_CAPACITY -- a host n beyond
 *             slot_keypoints.  Seen on the device only, by the first kernel, which raises one flag for the call: a count
 *             min(*d_n, n) beyond slot_keypoints (DVM_ERR_CAPACITY), a keypoint's octave outside [0, n_levels) (DVM_ERR_INVALID);
 *             the later kernels of the call then return at once, the error names the first such keyframe, and NO slot of the
 *             call is written: each keeps its content and its generation.
 *   put_tracked  put_device on frames frames[k] of the tracker's last finish, ordered behind dvm_orb_stream(h).  Accepted after a
 *             dvm_track_finish / dvm_track_finish_batch (any form) or after form (a) of dvm_track_reference_keyframe, until the
 *             tracker's next begin; the second-half and reference-keyframe calls in between do not end it.  DVM_ERR_STATE otherwise,
 *             and when h or its extraction is not the one the finish ran on; DVM_ERR_INVALID for a frame outside [0, count).  The
 *             camera, the bounds and the level tables are tables[k]'s (its d_* and n are ignored): nothing is read silently from the tracker.
 *   last_put_bytes  host-to-device bytes of the last put or put_device that reached the device.
 *   profile / last_put_ms  with profiling on, put_device records events around its launches; ms[0..3] = check, transform, bow, put of
 *             the last call's first round (a round: up to 32 keyframes).
 * sizeof(dvm_kfs_device_keyframe) == 96, sizeof(dvm_kfs_bow_out) == 56 (LP64). */
typedef struct {                 /* one keyframe whose arrays are in device memory */
  const dvm_keypoint* d_kps;     /* mvKeysUn, device */
  const uint8_t* d_desc;         /* n x 32, device */
  const int32_t* d_n;            /* device count (as dvm_orb_result_device), or NULL: n below is used */
  int32_t n;                     /* host count when d_n == NULL; else the capacity of the two arrays (count = min(*d_n, n)) */
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y;
  const float *scale_factors, *level_sigma2, *inv_level_sigma2;   /* host, [n_levels] */
  float log_scale_factor; int32_t n_levels;
} dvm_kfs_device_keyframe;
typedef struct {                 /* host buffers, each may be NULL; sized for slot_keypoints (+1 for fv_off) */
  int32_t n, n_bow, n_fv, n_feat;             /* written always */
  int32_t* bow_ids; double* bow_vals;         /* mBowVec, ascending word */
  int32_t *fv_node, *fv_off, *fv_feat;        /* mFeatVec as dvmh_vocab_transform returns it */
} dvm_kfs_bow_out;
int dvm_keyframe_store_put_device(dvm_keyframe_store* s, const dvm_vocab* voc, int levelsup, void* stream,
                                  int n, const int32_t* slots, const dvm_kfs_device_keyframe* kfs, dvm_kfs_bow_out* outs);
int dvm_keyframe_store_put_tracked(dvm_keyframe_store* s, dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, int levelsup,
                                   int n, const int32_t* frames, const int32_t* slots,
                                   const dvm_kfs_device_keyframe* tables /* scalars + level tables only; d_* and n ignored */,
                                   dvm_kfs_bow_out* outs);
int dvm_keyframe_store_last_put_bytes(const dvm_keyframe_store* s, int64_t* host_to_device);
int dvm_keyframe_store_profile(dvm_keyframe_store* s, int enable);
int dvm_keyframe_store_last_put_ms(const dvm_keyframe_store* s, float ms[4]);

/* ---- The Fuse chain on resident targets: dvm_fuse_targets_set_cam with every target given as a store slot plus what changes between
 * two LocalMapping steps, its pose.  The host fills the target table with pointers into the store and uploads that table alone: no
 * keypoint travels, no grid is built, no per-keypoint host loop runs.  dvm_fuse_targets_run / _run_hits are then used as they are.
 *   models  [n_targets] or NULL: the slots' own fx, fy, cx, cy (a zero one is DVM_ERR_INVALID); forms [n_targets] or NULL: as set_cam.
 *   A slot may appear in several targets of one set (rows are independent).  The set needs max_targets of dvm_fuse_targets_reserve
 *   only: max_total_target_keypoints may be 0.
 * Contract: for the same keyframes a run's rows equal dvm_fuse_targets_set_cam + run bit for bit -- both forms, both model types, mixed
 * targets, masks, run_hits: the search kernels read the same arrays in the same order.
 * The set records every named slot's generation: a run after one of them was put or removed is DVM_ERR_STATE ("a target's slot was
 * written since the set"), checked on the host; the handle stays usable -- set again.  A put to a slot the set does not name leaves it
 * valid.  A store on another device, a slot outside the store, never written or removed: DVM_ERR_INVALID before anything is queued. */
typedef struct { int32_t slot; dvm_se3f Tcw; float Ow[3]; } dvm_ft_target_resident;   /* 44 bytes */
int dvm_fuse_targets_set_resident(dvm_fuse_targets* h, const dvm_keyframe_store* store, int n_targets, const dvm_ft_target_resident* targets,
                                  const dvm_camera_model* models /* [n_targets], or NULL: the slots' fx, fy, cx, cy */,
                                  const uint8_t* forms /* [n_targets], or NULL: all DVM_FT_FORM_POINTS */);
/* The host-to-device bytes queued by the last set (uploaded or resident) and the last run; either pointer may be NULL. */
int dvm_fuse_targets_last_upload_bytes(const dvm_fuse_targets* h, int64_t* set_bytes, int64_t* run_bytes);

/* ---- The Fuse run on points named as map-store slots: dvm_fuse_targets_run / _run_hits with the point table read from the 72-byte
 * records of a dvm_map_store instead of travelling up.  ONE gather launch (k_ft_gather) fills the handle's point arrays from the records
 * -- position, normal, distance range, descriptor, and the row's valid flag -- and the search and hit kernels run as they are.
 *   Row i is searched iff slot[i] >= 0, (valid == NULL or valid[i]), records[slot[i]].bad == 0 and skip[t * n + i] is not set: isBad()
 *   is read on the device; skip stays the caller's IsInKeyFrame matrix.  A slot may appear more than once (its rows are equal).
 * Contract: for targets set by dvm_fuse_targets_set[_cam] or by dvm_fuse_targets_set_resident, the dense rows and the hits equal, bit for
 * bit, dvm_fuse_targets_run[_hits] on the table that dvm_map_store_read of those slots yields with `valid` as above -- both forms, both
 * model types, mixed targets.
 * Ordering: the gather and the search are bracketed as a reader of the store on the handle's stream: a run queued behind a
 * dvm_map_store_update, a dvm_ba_resident_commit or a dvm_map_store_refresh sees their bytes with no host synchronisation between, and a
 * later update waits for the run.
 * Bytes up per run: 4 n (+ n with valid) (+ T n with skip), each array rounded up to 64 (dvm_fuse_targets_last_upload_bytes).  n is
 * bounded by max_points of dvm_fuse_targets_reserve.
 * Errors, all decided on the host before anything is queued, the handle stays usable and no output array is written: those of
 * dvm_fuse_targets_run[_hits]; a NULL store where a slot is >= 0, a store on another device, a slot below -1, outside the capacity or
 * never written: DVM_ERR_INVALID.  n = 0 and T = 0 behave as in the uploaded run. */
typedef struct {
  const dvm_map_store* points;   /* the map the points live in; on the handle's device */
  int32_t n;
  const int32_t* slot;           /* [n] map-store slots; -1 = NULL pointer (the row is masked); a slot may appear more than once */
  const uint8_t* valid;          /* [n] or NULL (all) */
} dvm_ft_points_resident;        /* 32 bytes (LP64) */
int dvm_fuse_targets_run_resident(dvm_fuse_targets* h, const dvm_ft_points_resident* P, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist);
int dvm_fuse_targets_run_hits_resident(dvm_fuse_targets* h, const dvm_ft_points_resident* P, const uint8_t* skip, float th,
                                       int32_t* hit_off /* [T + 1] */, dvm_ft_hit* hits, int hit_cap, int32_t* n_hits);

/* ---- The second direction of SearchInNeighbors (src/LocalMapping.cc:826-846): vpFuseCandidates built and searched on the device.  The
 * call names the target keyframes' GetMapPointMatches() as map-store slots (4 B per keypoint, as dvm_kf_resident does); the device makes
 * the candidate list, gathers its records and searches it against the set targets in ONE chain with ONE synchronisation.
 *   The entries are numbered flat in (list, keypoint) order.  An entry is a candidate iff its slot is >= 0, its record is not bad and no
 *   earlier entry names the same slot; the candidates keep flat order.  A candidate whose slot is in `exclude` (the current keyframe's
 *   own list: IsInKeyFrame(mpCurrentKeyFrame)) stays in the list and its rows are masked.
 * Returns cand_slot[0 .. *n_cand) and the hits of the set targets against that list, hits[].point an index into cand_slot.  Both come
 * down through a mapped page-locked block: nothing of the size of the bound does.
 * Contract: cand_slot is the list defined above; hit_off and hits equal dvm_fuse_targets_run_hits_resident with P.slot = cand_slot and
 * skip[t * n + i] = (cand_slot[i] is in exclude).
 * dvm_fuse_targets_reserve_candidates: the first-index table of the dedupe (map_capacity words, idle between calls: every call puts it
 * back through the entries it touched) and the blocks for lists of up to max_entries entries in total (grow-only).  The call before it:
 * DVM_ERR_INVALID.  The flat length of the lists is the gather's and the search's n: beyond max_points of dvm_fuse_targets_reserve or
 * max_entries -- or n_exclude beyond max_entries, or a store of more than map_capacity slots -- DVM_ERR_CAPACITY before anything is
 * queued.  *n_cand > cand_cap: DVM_ERR_CAPACITY, *n_cand holds the full count and nothing is written past cand_slot[cand_cap); the hits
 * as in dvm_fuse_targets_run_hits; the handle stays usable.  Every list, exclude included, holds -1 or written slots of `points`
 * (otherwise DVM_ERR_INVALID before anything is queued).  sizeof(dvm_ft_candidates) == 48 (LP64). */
typedef struct {
  const dvm_map_store* points;
  int32_t n_lists;
  const int32_t* const* mp_slot;  /* [n_lists] a keyframe's GetMapPointMatches() as map-store slots, -1 = none */
  const int32_t* n;               /* [n_lists] their lengths */
  const int32_t* exclude;         /* [n_exclude] or NULL: the current keyframe's own mp_slot list (-1 entries ignored) */
  int32_t n_exclude;
} dvm_ft_candidates;
int dvm_fuse_targets_reserve_candidates(dvm_fuse_targets* h, int max_entries, int map_capacity);
int dvm_fuse_targets_run_hits_candidates(dvm_fuse_targets* h, const dvm_ft_candidates* C, float th,
                                         int32_t* cand_slot, int cand_cap, int32_t* n_cand,
                                         int32_t* hit_off /* [T + 1] */, dvm_ft_hit* hits, int hit_cap, int32_t* n_hits);

/* ---- CreateNewMapPoints on resident keyframes: dvm_create_new_map_points[_cam] with every keyframe given as a store slot plus its
 * per-call part -- mvpMapPoints (LocalMapping changes it between any two calls; 4 B per keypoint against about 70) and the pose.
 * Keypoints, descriptors, FeatureVector and level tables are read in the slots; the kernels are the uploaded call's.
 *   cur_model NULL: the pinhole chain on the slots' fx, fy, cx, cy (nb_models, nb_poses not read); otherwise the rules of
 *   dvm_create_new_map_points_cam.  The current keyframe's and the neighbours' slots are distinct keyframes (the precondition above).
 * Contract: the records equal dvm_create_new_map_points[_cam] on the same keyframes bit for bit; the reservation (its keypoint total
 * included), the baseline skip and the error rules are that call's own.  A keyframe put with fv_n = 0 is legal as cur or neighbour and
 * finds nothing, as a dvm_np_keyframe with fv_n = 0 does.  A slot outside the store, never written or removed, a NULL mp where the
 * slot holds keypoints, or a store on another device: DVM_ERR_INVALID before anything is queued. */
typedef struct { int32_t slot; const int32_t* mp; dvm_se3f Tcw, Twc; float Ow[3]; } dvm_np_keyframe_resident;   /* 88 bytes */
typedef struct { dvm_np_keyframe_resident kf; float median_depth; float ep[2], F12[9]; } dvm_np_neighbour_resident;   /* 136 bytes */
int dvm_create_new_map_points_resident(dvm_new_points* h, const dvm_keyframe_store* store, const dvm_np_keyframe_resident* cur,
                                       const dvm_camera_model* cur_model /* NULL: pinhole from the slots */, int n_neighbours,
                                       const dvm_np_neighbour_resident* nbs, const dvm_camera_model* nb_models, const dvm_pair_pose* nb_poses,
                                       const dvm_np_params* p, dvm_np_out* out);
/* The host-to-device bytes queued by the last call that reached the device, resident or not. */
int dvm_new_points_last_upload_bytes(const dvm_new_points* h, int64_t* bytes);

/* ---- A resident keyframe, as the place-recognition searches and TrackReferenceKeyFrame name it (below): a keyframe-store slot plus
 * GetMapPointMatches() as map-store slots, 4 B per keypoint.  Descriptors, mvKeysUn and the FeatureVector are read in the slot; the
 * map points' isBad(), Observations() and GetWorldPos() in the 72-byte records of `points`.  Different keyframes of one call may name
 * different map stores (merge candidates belong to other maps); all of them, and the keyframe store, live on the handle's device.
 * An mp_slot is -1 or a written slot of `points`; anything else is DVM_ERR_INVALID.  sizeof(dvm_kf_resident) == 24 (LP64). */
typedef struct {
  int32_t slot;                 /* dvm_keyframe_store slot */
  const dvm_map_store* points;  /* the map this keyframe's points live in; may be NULL when every mp_slot is -1 */
  const int32_t* mp_slot;       /* [n of the slot] GetMapPointMatches() as map-store slots, -1 = NULL pointer */
} dvm_kf_resident;

/* ---- dvm_search_by_bow_targets on resident keyframes.  The keyframe table's desc / fv_node / fv_off / fv_feat point into the slots;
 * the mp_slot lists are the whole per-keypoint upload.  ONE prologue launch (k_bt_prologue) then writes into the handle's device block,
 * for every keyframe of the call, use[i] = mp_slot[i] >= 0 && !record.bad and angle[i] = the slot's mvKeysUn[i].angle, -1 into every
 * match row (a feature of cur that no node lists keeps it: no host pass) and zero into the per-target counters; the search and the
 * settle kernels are the uploaded call's.  The search is ordered behind every put to `kfs` and every update of a named map store
 * queued before the call, and a put or update queued after it waits for it.
 * Contract: for the same keyframes match_idx2 and nmatches equal dvm_search_by_bow_targets bit for bit, where that call carries
 * mp[i] = mp_slot[i] and bad[i] = the record's bad != 0.
 * Upload: exactly
 *     64 * ceil(56 * (T + 1) / 64) + 64 * ceil(32 * (T + 1) / 64) + sum over cur and the T targets of 64 * ceil(4 * n / 64)
 * bytes (the keyframe table, the prologue's table, the lists) -- at most 4 B per keypoint, each list rounded up to 64 B, plus 256 B per
 * keyframe.  dvm_bow_targets_last_upload_bytes reports it, for either form.
 * dvm_bow_targets_reserve keeps its meaning: max_total_target_keypoints bounds the device block, which holds the flags and angles.
 * The listed-once rule (a feature lies in ONE node) is checked per call by the uploaded form; dvm_keyframe_store_put accepts such a
 * keyframe as before and records per slot whether the rule holds; this call refuses a slot where it does not.
 * Errors, all before anything is queued, the handle stays usable, each naming the keyframe: DVM_ERR_INVALID -- a slot outside the
 * store, never written or removed; a store on another device; an mp_slot below -1, outside its map store or never written; a NULL
 * mp_slot where the slot holds keypoints; a NULL points with an mp_slot >= 0; a slot whose FeatureVector lists a feature twice.
 * DVM_ERR_CAPACITY -- beyond the reservation.  Legal, as in the uploaded call: n_targets = 0, a keyframe with n = 0 or fv_n = 0, one
 * slot as cur and as a target, one slot as several targets under different mp_slot lists. */
int dvm_search_by_bow_targets_resident(dvm_bow_targets* h, const dvm_keyframe_store* kfs, const dvm_kf_resident* cur, int n_targets,
                                       const dvm_kf_resident* targets, float nnratio, int check_ori, int32_t* match_idx2, int32_t* nmatches);
/* The host-to-device bytes queued by the last call that reached the device, either form. */
int dvm_bow_targets_last_upload_bytes(const dvm_bow_targets* h, int64_t* bytes);
/* With dvm_bow_targets_profiling on: the prologue kernel's milliseconds of the last call (0 after an uploaded call). */
int dvm_bow_targets_last_prologue_ms(dvm_bow_targets* h, float* ms);

/* ---- The first half reading a store: dvm_track_finish_batch with the projection queries built ON THE DEVICE (k_track_queries) from
 * LastFrame's entry list -- the loop header of ORBmatcher.cc:1573-1611, what dvmh_track_with_motion_model builds on the host: x3Dc = Tcw *
 * pos (Sophus' quaternion form), invzc = (float)(1.0 / z) with invzc < 0 skipped, the projection through the tracker's camera model, the
 * four bound tests, radius = th * scale_factors[octave], levels octave - 1 .. octave + 1; the kept entries compacted in entry order (the
 * claim replay is sequential in that order).  Per entry the host sends 9 bytes (slot, octave, angle) instead of a 69-byte query and
 * projects nothing.  Behind the builder the chain is dvm_track_finish_batch's, with its state rules and statuses; count == 1 is the
 * single frame; it may be called again after one begin (the wider attempt changes th only).
 *   outs[b].assign[j] is the ENTRY NUMBER in last[b] matched to keypoint j, or -1: the caller's map point is slot[assign[j]].
 *   last[b].n beyond the tracker's max_queries: DVM_ERR_CAPACITY.  A NULL array with n > 0, an octave >= p->nlevels, a store on another
 *   device, a slot outside its store or never written: DVM_ERR_INVALID, before anything is queued (the begin stays valid).
 *   Camera: pinhole fx * x / z + cx in float on (float)p->cam; under a KannalaBrandt8 tracker (dvm_tracker_set_camera_model)
 *   dvm_cam::kb8_project on the tracker's model, and p->cam is not read.  Pinhole queries equal the host's bit for bit; KannalaBrandt8
 *   queries differ where the device's atan2f and libm's differ in the last bit of theta. */
typedef struct {
  const dvm_map_store* store;      /* this agent's map points (may be NULL when n == 0) */
  int32_t n;                       /* LastFrame entries that hold a map point and are not outliers, ascending keypoint index */
  const int32_t* slot;             /* [n] store slot of the entry's map point */
  const uint8_t* octave;           /* [n] LastFrame.mvKeys[i].octave */
  const float* angle;              /* [n] LastFrame.mvKeysUn[i].angle */
  dvm_se3f Tcw_pred;               /* mVelocity * mLastFrame.GetPose() */
  float th;                        /* SearchByProjection's th of THIS call (15, or 30 on the wider attempt) */
} dvm_track_last;                  /* 72 bytes */
typedef struct {                   /* what the frames of a call share: the fields of dvm_track_queries that are not per query */
  float bounds[4]; const dvm_distortion* dist; const float* scale_factors; const float* inv_level_sigma2; int32_t nlevels;
  dvm_ba_camera cam; int32_t th_high, check_ori, min_matches;
} dvm_track_shared;                /* 104 bytes */
int dvm_track_finish_batch_resident(dvm_tracker* t, dvm_orb* h, int count, const dvm_track_last* last, const dvm_track_shared* p,
                                    const dvm_track_frame_out* outs, dvm_track_result* res);
/* Test hook: k_track_queries alone on the tracker's own stream -- no begin, no image, the tracker's state untouched -- and the block copied
 * back.  *stride = the call's per-query stride (the largest n rounded up to 64, at least 64); frame b's arrays begin at b * *stride
 * elements (qdesc: x 32, q_pos: x 3), so every array holds count * stride elements; nq [count].  p->th_high / check_ori / min_matches and
 * p->dist are not read. */
int dvm_track_debug_build_queries(dvm_tracker* t, int count, const dvm_track_last* last, const dvm_track_shared* p, int32_t* nq,
                                  int32_t* q_entry, float* qx, float* qy, float* qr, int32_t* qmin, int32_t* qmax, uint8_t* q_claims,
                                  float* q_angle, float* q_pos, uint8_t* qdesc, int32_t* stride);
/* The host-to-device bytes queued by the tracker's last finish (first_half) and last local-map call (second_half), resident or not: the
 * query block or entry lists, tables or slot lists, with their per-frame parameters (the images are the extractor's and not counted).
 * Either pointer may be NULL. */
int dvm_tracker_last_upload_bytes(const dvm_tracker* t, int64_t* first_half, int64_t* second_half);

/* ---- The second half reading stores: dvm_track_local_map_batch with every frame's table given as store slots (4 B per point instead of
 * 72).  A gather kernel (k_store_gather) fills the chain's device table at the frames' offsets from the stores; everything behind it is
 * dvm_track_local_map_batch's chain, and reservation, state rules, skipped frames, track_pts and outputs are exactly its own.  Accepted
 * after either finish, resident or uploaded.  frame_mp and the outputs index the slot list (table positions), as they index pts there.
 * A slot outside its store or never written, or a store on another device: DVM_ERR_INVALID before anything is queued. */
typedef struct {
  const dvm_map_store* store; const int32_t* slots; int32_t n;   /* mvpLocalMapPoints as store slots; n may be 0 */
  const int32_t* frame_mp;                                       /* [N_b] index into slots (table position) or -1 */
  float th; int32_t far_points; float th_far;
} dvm_local_map_in_resident;                                     /* 48 bytes */
int dvm_track_local_map_batch_resident(dvm_tracker* t, dvm_orb* h, int count, const dvm_local_map_in_resident* in,
                                       const dvm_local_map_out* out, dvm_track_local_result* res, int32_t* status);

/* ---- The other way into TrackLocalMap, Tracking::TrackReferenceKeyFrame (src/Tracking.cc:2461-2520), as ONE device chain: taken by
 * Tracking::Track (:1756-1765) when there is no motion model (no velocity yet, or within two frames of a relocalisation) or when
 * TrackWithMotionModel failed.  Frame::ComputeBoW (DBoW2 transform, levelsup 4) -> ORBmatcher(0.7, true).SearchByBoW(mpReferenceKF, F)
 * (src/ORBmatcher.cc:214-393) -> Optimizer::PoseOptimization seeded from mLastFrame.GetPose() (src/Optimizer.cc:744-1028) -> outlier
 * matches dropped, nmatchesMap (:2486-2516).  The frame's descriptors and grid stay on the device; the keyframe goes up in one
 * asynchronous copy; one synchronisation at the end.  Results equal dvm_orb_extract + dvmh_vocab_transform +
 * dvmh_search_by_bow_kf_frame + dvm_pose_optimize composed in that order, bit for bit. */
typedef struct {
  int32_t n;                       /* mpReferenceKF->N */
  const dvm_keypoint* kps_un;      /* [n] mvKeysUn (the angle is what SearchByBoW reads) */
  const uint8_t* desc;             /* [n][32] mDescriptors */
  const int32_t* mp;               /* [n] the caller's map-point id from GetMapPointMatches(), or -1 */
  const float* mp_pos;             /* [n][3] GetWorldPos() of that point (read where mp >= 0) */
  const int32_t* mp_nobs;          /* [n] Observations() */
  const uint8_t* mp_bad;           /* [n] isBad(), or NULL */
  int32_t fv_n;                    /* mFeatVec flattened as dvmh_feature_vector_view: fv_n nodes, ascending as unsigned */
  const int32_t *fv_node, *fv_off, *fv_feat;   /* [fv_n], [fv_n + 1], [fv_off[fv_n]] */
} dvm_ref_keyframe;                /* 88 bytes */
typedef struct {
  double pose_in[7];               /* mLastFrame.GetPose() widened to double (tx ty tz qx qy qz qw), as dvm_track_queries::pose_in */
  float nnratio;                   /* 0.7 */
  int32_t check_ori;               /* 1 */
  int32_t th_low;                  /* ORBmatcher::TH_LOW (50) */
  int32_t min_matches;             /* 15 (Tracking.cc:2470) */
  int32_t min_map;                 /* 10 (Tracking.cc:2519) */
  int32_t levelsup;                /* ComputeBoW's levelsup (4) */
  float bounds[4];                 /* as dvm_track_queries: form (a) builds the grid with them */
  const dvm_distortion* dist;      /* NULL or k1 == 0: mvKeysUn = mvKeys (form (a)) */
  const float* inv_level_sigma2;   /* mvInvLevelSigma2, nlevels entries */
  int32_t nlevels;
  dvm_ba_camera cam;               /* fx fy cx cy of PoseOptimization's edges */
} dvm_track_refkf_params;          /* 160 bytes */
typedef struct {
  dvm_keypoint* kps; uint8_t* desc; int32_t cap;   /* [cap] form (a): the extraction (as dvm_orb_extract); may be NULL in form (b) */
  dvm_keypoint* kps_un;                            /* [cap] or NULL: mvKeysUn (form (a)) */
  int32_t* mp_out;                                 /* [N] mvpMapPoints after the outlier drop: the caller's ids, or -1 */
  int32_t* dropped;                                /* [N] the id whose match PoseOptimization rejected, or -1 (mbTrackInView /
                                                      mnLastFrameSeen of :2491-2503) */
  uint8_t* outlier;                                /* [N] mvbOutlier as PoseOptimization leaves it (before the drop resets it) */
  int32_t* bow_ids; double* bow_vals;              /* [N] or NULL: mBowVec (n_bow entries, ascending word) */
  int32_t *fv_node, *fv_off, *fv_feat;             /* [N], [N + 1], [N] or NULL: mFeatVec (n_fv nodes), as dvmh_vocab_transform */
} dvm_track_refkf_out;             /* 96 bytes */
typedef struct {
  int32_t n, mono_index;           /* the extraction's keypoint count and monoIndex */
  int32_t status;                  /* DVM_TRACK_COMPLETE; FEW_MATCHES: nmatches < min_matches (no optimisation, pose = pose_in);
                                      FEW_MAP_MATCHES: nmatchesMap < min_map */
  int32_t nmatches;                /* SearchByBoW's return value */
  int32_t nmatches_before_rotation;
  int32_t n_edges, n_inliers;      /* PoseOptimization: nInitialCorrespondences and its return value */
  int32_t nmatches_after;          /* nmatches after the outlier drop */
  int32_t nmatches_map;            /* nmatchesMap */
  int32_t n_bow, n_fv;             /* entries of mBowVec, nodes of mFeatVec */
  int32_t reserved;
  double pose[7];                  /* the optimised Tcw (tx ty tz qx qy qz qw) */
  dvm_se3f Tcw;                    /* the same as SetPose receives it */
  int32_t reserved2;
} dvm_track_refkf_result;          /* 136 bytes */
/* Allocates the chain's working set for reference keyframes of up to max_kf_keypoints keypoints (the keyframe upload, the frame's BoW
 * arrays, the match state), once; a single-frame tracker of at most 8 192 keypoints.  Called again, it replaces the working set;
 * dvm_tracker_destroy frees it. */
int dvm_tracker_reserve_reference_keyframe(dvm_tracker* t, int max_kf_keypoints);
/* Accepted once per dvm_track_begin on a single-frame tracker (dvm_tracker_create), same tracker and extractor (otherwise DVM_ERR_STATE):
 *   (a) right after dvm_track_begin, no finish: the no-motion-model case.  The call does what dvm_track_finish does before its search
 *       (undistortion when k1 != 0, the grid) and returns kps / desc / kps_un as dvm_track_finish does;
 *   (b) right after a dvm_track_finish of that frame, whatever its status: the motion-model-failed case.  Nothing of the first half's
 *       matches or pose carries over.
 * kf->n beyond the reservation: DVM_ERR_CAPACITY.  After DVM_TRACK_COMPLETE, dvm_track_local_map is accepted on the frame (the grid and
 * mvKeysUn this call left, seeded from this call's pose); after any other status it is refused. */
int dvm_track_reference_keyframe(dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, const dvm_ref_keyframe* kf, const dvm_track_refkf_params* p,
                                 dvm_track_refkf_out* out, dvm_track_refkf_result* res);
/* The working set of dvm_track_reference_keyframe_batch, separate from dvm_tracker_reserve_reference_keyframe's and accepted on any tracker:
 * max_total_kf_keypoints is the TOTAL of one call, the sum over its keyframes of n (of fv_n where that is larger), each rounded up to 64
 * (up to max_frames x 8 192); the per-frame arrays are reserved for max_frames frames.  DVM_ERR_CAPACITY for what it cannot hold.  Called
 * again, it replaces the working set; dvm_tracker_destroy frees it. */
int dvm_tracker_reserve_reference_keyframe_batch(dvm_tracker* t, int max_total_kf_keypoints);
/* TrackReferenceKeyFrame for the frames of one camera tick (several agents on one GPU) that need it: after the batched first half, the
 * frames whose motion model failed or that had none (the caller passed nq = 0 queries: DVM_TRACK_FEW_MATCHES) run ComputeBoW ->
 * SearchByBoW -> PoseOptimization as ONE chain of batched launches: one upload of all keyframes, one synchronisation.  Accepted right after a
 * dvm_track_finish_batch of `count` frames (or a dvm_track_finish: count = 1) on the same tracker and extractor, once per finish (otherwise
 * DVM_ERR_STATE; where the finish ran twice, the last one counts).  kfs / ps / outs / res / status: `count` entries.
 *   kfs[b] != NULL: form (b) of dvm_track_reference_keyframe on frame b whatever its first-half status -- res[b] and outs[b] exactly what
 *     that call gives on the frame alone; status[b] = res[b].status.  outs[b].kps / desc / kps_un are not written (the finish returned them).
 *   kfs[b] == NULL: status[b] = the first half's status, res[b] zeroed, outs[b] not written, ps[b] not read.
 * ps[b].pose_in is per frame; nnratio, check_ori, th_low, min_matches, min_map, levelsup, the level table and cam must be equal across the
 * frames that run (DVM_ERR_INVALID); bounds and dist are not read.  Every keyframe is checked as the single call checks it before anything
 * runs; the keyframes' total beyond the reservation: DVM_ERR_CAPACITY.  A refused call leaves the finish for a corrected one.  Afterwards
 * dvm_track_local_map_batch (count frames) treats a frame as complete when status[b] == DVM_TRACK_COMPLETE, seeded from this call's pose
 * where the frame ran; with count = 1, dvm_track_local_map is accepted as after dvm_track_reference_keyframe.  DVM_TRACK_BATCH_TIMING=1
 * prints the call's host phases on stderr. */
int dvm_track_reference_keyframe_batch(dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, int count, const dvm_ref_keyframe* const* kfs,
                                       const dvm_track_refkf_params* ps, const dvm_track_refkf_out* outs, dvm_track_refkf_result* res,
                                       int32_t* status);
/* dvm_track_reference_keyframe_batch on resident keyframes: kf[b] names frame b's reference keyframe as a slot of `kfs` plus its map
 * points as map-store slots (dvm_kf_resident above), NULL = the frame does not run.  The host uploads the mp_slot lists and the small
 * per-frame arrays and nothing per keypoint beyond those 4 B; a gather kernel (k_refkf_gather, one workgroup per frame that runs)
 * packs the chain's keyframe block on the device -- descriptors and the FeatureVector out of the slot, the angle out of its keypoint
 * records, and per keypoint out of the map point's record use = id >= 0 && !bad, claims = id >= 0 && n_obs > 0, pos = id >= 0 ?
 * record.pos : 0.  Everything behind the gather is the uploaded call's chain; it is ordered behind every put and update queued before.
 * Contract: state rules, reservation (dvm_tracker_reserve_reference_keyframe_batch: a slot counts its n rounded up to 64), skipped
 * frames, outputs and statuses are dvm_track_reference_keyframe_batch's, the call that follows is accepted as after it, and res, outs
 * and status equal that call's bit for bit where it carries mp = mp_slot and mp_pos / mp_nobs / mp_bad read from the records -- under
 * the pinhole tracker and a KannalaBrandt8 one; outs[b].mp_out / dropped hold map-store slots.  count = 1 on a single-frame tracker
 * is legal.  DVM_ERR_INVALID before anything is queued, the finish left for a corrected call: a slot outside the store, never written
 * or removed; a store on another device; an mp_slot below -1, outside its map store or never written; a NULL mp_slot where the slot
 * holds keypoints; a NULL points with an mp_slot >= 0.  DVM_ERR_CAPACITY: the keyframes' total beyond the reservation. */
int dvm_track_reference_keyframe_batch_resident(dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, const dvm_keyframe_store* kfs, int count,
                                                const dvm_kf_resident* const* kf /* [count], NULL = frame does not run */,
                                                const dvm_track_refkf_params* ps, const dvm_track_refkf_out* outs,
                                                dvm_track_refkf_result* res, int32_t* status);
/* The host-to-device bytes queued by the tracker's last reference-keyframe call that reached the device, any form. */
int dvm_tracker_last_refkf_upload_bytes(const dvm_tracker* t, int64_t* bytes);

/* Optimizer::OptimizeSim3 (Optimizer.cc:1960-2212), numerics for N correspondences gathered by the caller:
 * P1c / P2c = the matched map points in their own key frame's camera frame (R1w*P+t1w, R2w*P+t2w), obs1 / obs2 =
 * undistorted keypoints in KF1 / KF2, w1 / w2 = mvInvLevelSigma2[octave], K1 / K2 = (fx,fy,cx,cy) of both pinhole
 * cameras, th2 = chi-square gate (Huber delta = sqrt(th2)).  S12 (in/out) = (qx,qy,qz,qw, tx,ty,tz, s) = g2o::Sim3.
 * Runs optimize(5) -> inlier test -> kernels off -> optimize(5|10) -> final test on the device (one workgroup).
 * inlier[N] = 1 for surviving pairs; *n_inliers = the reference's return value (0 if < 10 pairs survive round 1).
 * Host pointers, synchronous. */
int dvm_optimize_sim3(int device, double* S12, int fix_scale, const double* P1c, const double* P2c, const double* obs1,
                      const double* obs2, const double* w1, const double* w2, int N, const double* K1, const double* K2,
                      double th2, uint8_t* inlier, int32_t* n_inliers);

/* dvm_optimize_sim3 on a camera model per keyframe (EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ project with pCamera1 / pCamera2,
 * OptimizableTypes.h:183, 202): model1 / model2 = the cameras of KF1 / KF2, their p[0..3] replace K1 / K2; all four pairs of (pinhole,
 * KannalaBrandt8) are accepted.  For a KannalaBrandt8 keyframe obs are mvKeysUn = mvKeys.  Arguments, outputs and return values are
 * otherwise dvm_optimize_sim3's; with model 0 on both sides the outputs are dvm_optimize_sim3's bit for bit.
 * On a KannalaBrandt8 side the projection is split:
 *   - the residual and every chi2 test (Huber weights, the inlier tests of both rounds, the final count) take the reference's
 *     project(Vector3d): theta from the FLOAT atan2f / sqrtf (KannalaBrandt8.cpp:48-51), so the residual is a step function of the state
 *     with steps of one float ulp of theta (~3e-8 rad);
 *   - the numeric Jacobian is the same central difference at delta = 1e-9 through the same 28 perturbed states, taken on the projection
 *     with theta from the DOUBLE atan2 (camera_model.h: kb8_project_exact), e = obs - proj in the pinhole path's operand order.
 * g2o's own numeric Jacobian through the float theta is 0 almost everywhere -- a 1e-9 perturbation crosses a step in a few per cent of the
 * evaluations -- with spikes of ~1e-5 px / 2e-9, several thousand px per unit, where it does: a result that hangs on libm's last bit of
 * atan2f.  Nothing can be pinned to that and nobody wants it, so this entry departs from the reference here, as bundle adjustment on a
 * camera model does (residual from the quantised project, Jacobian from projectJac's double atan2).  The pinhole path is untouched.
 * DVM_ERR_INVALID, before anything runs and before the device is touched, for a NULL model, a model outside {0, 1} or a zero focal length. */
int dvm_optimize_sim3_cam(int device, double* S12, int fix_scale, const double* P1c, const double* P2c, const double* obs1,
                          const double* obs2, const double* w1, const double* w2, int N, const dvm_camera_model* model1,
                          const dvm_camera_model* model2, double th2, uint8_t* inlier, int32_t* n_inliers);

/* Optimizer::OptimizeEssentialGraph numerics (src/Optimizer.cc:1389-1652): Sim3 pose graph of n vertices
 * (S[n][8] = estimates Siw as (q_xyzw, t, s), in/out; fixed[v] != 0 keeps a vertex) and E EdgeSim3 (vertex 0 = vi,
 * vertex 1 = vj, measurement Sji = Sjw * Swi, information = identity).  g2o's numeric Jacobians, Levenberg-Marquardt
 * with lambda_init 1e-16, `iterations` = optimize(20) in the reference.  Which keyframes / edges enter the graph and the
 * SE3 / map-point correction afterwards (:1601-1648) stay with the caller.  Host pointers, synchronous. */
typedef struct { int32_t vi, vj; double Sji[8]; } dvm_pg_edge;
typedef struct {
  int32_t iterations, total_trials, stop_reason, levels;
  double chi2_initial, chi2_final, lambda_final, tile_fill, ms_structure, ms_optimize;
  double chi2_per_iter[32];   /* chi2 after each outer iteration (first 32) */
  int32_t trials_per_iter[32];
} dvm_pg_stats;
int dvm_pose_graph_optimize(int device, double* S, const uint8_t* fixed, int n, const dvm_pg_edge* edges, int E,
                            int fix_scale, int iterations, dvm_pg_stats* stats);

/* Test hook (tests/test_gpu_pose_graph.py): ONE Levenberg-Marquardt trial of dvm_pose_graph_optimize at a caller-given lambda,
 * through the same set-up and the same launches, with every stage handed back.  nfree = number of vertices with fixed[v] == 0;
 * "free vertex a" = the a-th of them by vertex id.  Outputs (host, caller-allocated):
 *   e[E][7], J[E][2][49] (side 0 = vertex i, side 1 = vertex j; row-major [error row][dof]) and chi2_before at the input state;
 *   H[7 nfree][7 nfree] row-major: the lower triangle of J^T J + lambda I, b[7 nfree] = -J^T e (the augmented rhs row the
 *   factorisation reads) and the solution x[7 nfree], all in vertex-id order of the free vertices (the elimination order and the
 *   tile layout are undone here); vidx[n] = position of each vertex in the elimination order (-1 = fixed);
 *   S = the estimates after oplus, scale_sum = computeScale's x^T (lambda x + b), chi2_after at the new estimates.
 * failed != 0: the factorisation met a non-positive pivot; x keeps its initial zeros and S comes back as it was (normalised). */
typedef struct {
  int32_t nfree, failed, levels, reserved;
  double chi2_before, chi2_after, scale_sum;
} dvm_pg_trial_stats;
int dvm_pose_graph_debug_trial(int device, double* S, const uint8_t* fixed, int n, const dvm_pg_edge* edges, int E, int fix_scale,
                               double lambda, double* e, double* J, double* H, double* b, double* x, int32_t* vidx,
                               dvm_pg_trial_stats* stats);

/* Test hook (tests/test_gpu_tile_solve.py): ONE linear system through the tile Cholesky that solves the bundle adjustment's reduced system
 * and the pose graph's normal equations, with no edge, camera or Levenberg-Marquardt step around it: the same schedule (ba_tile_schedule), the
 * same set-up of the solver's members, the same launcher.  Host pointers, synchronous.
 * The system, in unknown space and elimination order: n_blocks blocks of dof rows, per_tile to a 64-row tile ((dof, per_tile) = (6, 10) or
 * (7, 9)), then n_kept blocks of 3 rows, 21 to a tile (kept landmark j = landmark kept_list[j] of n_landmarks, each listed once);
 * n = dof * n_blocks + 3 * n_kept.  A[n][n] row-major, symmetric positive definite, lower triangle read; b[n];
 * mask[tiles][tiles] (lower triangle read): the structurally non-zero tiles -- a tile may be present and hold zeros, a non-zero of A outside
 * the mask is refused -- or null: the tiles where A (or A2) is not zero (either way all of A is read on the host, O(n^2), with the other
 * argument checks and before a device is looked for).  x_in[dof * n_blocks + 3 * n_landmarks]: what x holds before each solve.
 * form: 0 = level launches as the bundle adjustment sets them up by default (top pair when the schedule has one, diagonal tiles inside the
 * level launches, n_root_raw honoured, in-launch hand-offs), changed by the DVM_TILE_FORM_* bits; a flow form that the admission test
 * forbids (info->flow_refusal & 7) is an error, never a silent fall-back.
 * repeats (1..8): the system is solved that many times on the same structure, S rewritten and x reset to x_in before each solve, the
 * sequence number of the hand-off flags increasing; with A2 / b2 (both or neither; same mask) that second system is solved in between.
 * Outputs: x[repeats][dof * n_blocks + 3 * n_landmarks] (unknown block i at dof * i, landmark l at dof * n_blocks + 3 * l), fail[repeats]
 * (non-zero: a non-positive pivot, x keeps x_in), x2 / fail2 (null, or [repeats - 1] of the same): the solves of A2 in between; info: the
 * schedule and, for the first solve, what the launcher launched. */
#define DVM_TILE_FORM_FLOW 1              /* k_chol_flow: factorisation and back substitution in one launch */
#define DVM_TILE_FORM_NO_PAIR 2           /* the top pair goes through the level launches, not k_chol_pair */
#define DVM_TILE_FORM_NO_DIAG_IN_LEVEL 4  /* diagonal tiles by k_chol_diag, never inside a level launch */
#define DVM_TILE_FORM_NO_ROOT_RAW 8       /* the root columns' panel solve is launched, not left to the back substitution */
#define DVM_TILE_FORM_PER_PHASE 16        /* no in-launch hand-offs: one launch per phase, the pose graph's form */
/* level_path[h]: what was launched for level h */
#define DVM_TILE_PATH_NONE 0                /* nothing: the rhs tile's level, the top pair's levels, every level of the flow form */
#define DVM_TILE_PATH_LEVEL_ONE_LAUNCH 1    /* the whole level, diagonal tiles included, in one launch */
#define DVM_TILE_PATH_SLICES_DIAG_UPDATE 2  /* panel slices with the diagonal tiles in one launch, the trailing update behind it */
#define DVM_TILE_PATH_DIAG_FUSED 3          /* diagonal tiles, then panel solves + trailing update in one launch */
#define DVM_TILE_PATH_DIAG_TRSM_UPDATE 4    /* diagonal tiles, panel solves, trailing update: one launch each */
#define DVM_TILE_PATH_RAW_ROOT 5            /* diagonal tiles alone; the back substitution does the panel solve */
typedef struct {
  int32_t n_tiles, levels, pair_a, pair_b, n_root_raw, flow_leaves, roots, flow_tasks;
  int32_t flow_refusal;      /* 1 S too large, 2 several roots, 4 too many leaves for the workgroups, 8 the level launches are preferred */
  int32_t traced_levels, used_pair, used_flow, backsolve_cols, reserved;
  int32_t level_nc[64], level_ns[64], level_nt[64];   /* columns, strips and trailing targets per level (first 64) */
  int32_t level_path[64];
} dvm_tile_solve_info;
int dvm_tile_solve_debug(int device, int n_blocks, int dof, int per_tile, int n_kept, const int32_t* kept_list, int n_landmarks,
                         const double* A, const double* b, const uint8_t* mask, const double* x_in, int form, int repeats,
                         const double* A2, const double* b2, double* x, int32_t* fail, double* x2, int32_t* fail2, dvm_tile_solve_info* info);
/* Test hook, host only (no device needed): the schedule of a tile mask over n_tiles tiles of unknowns as dvm_tile_solve_debug would
 * build it, with the flow form's admission test for `workgroups` compute units.  Fills the schedule part of info.  n_tiles <= 256: the
 * symbolic factorisation keeps dense per-level maps, fine for a test and for nothing larger. */
int dvm_tile_schedule_debug(int n_tiles, const uint8_t* mask, int workgroups, dvm_tile_solve_info* info);

/* Sim3Solver::ComputeSim3 + CheckInliers (src/Sim3Solver.cc:294-408) for H RANSAC hypotheses in one launch.
 * P1c / P2c: the N matched map points in the two keyframes' camera frames (mvX3Dc1 / mvX3Dc2, float[3N]);
 * max_err1/2: mvnMaxError1/2 as the reference stores them, (float)(size_t)(9.210 * sigma2); K1 / K2: fx, fy, cx, cy;
 * triples: the minimal sets (3 correspondence indices each; the reference draws them with DUtils::Random, :171-181).
 * Outputs per hypothesis: T12[13] = {s12, R12 row-major, t12}, n_inliers, inlier_mask[N].  The sequential
 * best-hypothesis rule of iterate() (:154-185) stays with the caller.  Host pointers, synchronous. */
int dvm_sim3_hypotheses(int device, const float* P1c, const float* P2c, const float* max_err1, const float* max_err2, int N,
                        const float* K1, const float* K2, const int32_t* triples, int H, int fix_scale, float* T12,
                        int32_t* n_inliers, uint8_t* inlier_mask);
/* dvm_sim3_hypotheses on a camera model per keyframe: the four projections of CheckInliers and FromCameraToImage are
 * pCamera1->project / pCamera2->project(Vector3f) (Sim3Solver.cc:393-394, 422-446) of model1 / model2, whose p[0..3] replace K1 / K2;
 * all four pairs of (pinhole, KannalaBrandt8).  Horn's closed form reads no camera: T12 is dvm_sim3_hypotheses' bit for bit under every
 * pair, and with model 0 on both sides so are the counts and the masks.  DVM_ERR_INVALID, before anything runs and before the device
 * is touched, for a NULL model, a model outside {0, 1} or a zero focal length. */
int dvm_sim3_hypotheses_cam(int device, const float* P1c, const float* P2c, const float* max_err1, const float* max_err2, int N,
                            const dvm_camera_model* model1, const dvm_camera_model* model2, const int32_t* triples, int H,
                            int fix_scale, float* T12, int32_t* n_inliers, uint8_t* inlier_mask);

/* ---- LocalBundleAdjustment on the resident stores: dvm_ba_optimize_windows_fast[_cam] whose observations and points are READ from the
 * keyframe slots and the map slots they have been lying in since ComputeBoW, and whose result goes BACK into the map slots on the device.
 *   optimize  the cluster form (k_ba_window_cluster<CAM>, unchanged) on K windows.  Per observation only the 12-byte dvm_ba_obs goes up,
 *             per point its slot (and ref_edge): a gather kernel in front of the solver fills, in the tables' sorted edge order,
 *             e_obs = (double)mvKeysUn[kp].pt, e_info = (double)mvInvLevelSigma2[octave] from the slot of the edge's camera and
 *             pts = (double)record[mp_slot].pos (the casts of Optimizer.cc:1188, 1207-1217).  poses, points, edge_chi2, depth_positive
 *             and the statistics are those of dvm_ba_optimize_windows_fast (models NULL) / _fast_cam on the host-gathered window, bit
 *             for bit.  The windows of one call may name different keyframe stores and different map stores (K agents).  Behind the
 *             solver a prepare step leaves in memory of the handle, per window: the cameras' centres as float -- a free camera's from
 *             its optimised pose as SE3f(Quaternionf, Vector3f).inverse().translation() (Optimizer.cc:1374, SetPose's mOw), a fixed
 *             camera's the caller's ow row or, without one, the same of its input pose without the constructor's normalisation --; per
 *             point whether it is DIRTY (one of its edges has chi2 > chi2_erase or no positive depth, Optimizer.cc:1324) or UNUSED (no
 *             edge); and for every clean, used point SetWorldPos + MapPoint::UpdateNormalAndDepth (MapPoint.cc:473-540) in float32:
 *             pos = (float)points_out, normal = mean over the point's edges IN THE CALLER'S ORDER of (pos - ow) / |pos - ow|,
 *             max_dist = |pos - ow[ref]| * scale_factors[octave of the ref keypoint], min_dist = max_dist / scale_factors[n_levels - 1]
 *             (tables of the ref keyframe's slot).  geometry_out rows of dirty and unused points are zeros; without ref_edge
 *             min_dist = max_dist = 0.  Runs outside the map mutex, as Optimizer.cc:1311 does; synchronous.  DVM_BA_SPLIT is not honoured.
 *   commit    window k of the last optimize (-1: every window not yet committed): ONE scatter per distinct map store, queued as
 *             dvm_map_store_update queues its own -- on the store's stream, behind the last kernel queued to read the store, followed by
 *             the store's write event; it does not wait.  It writes pos, normal, min_dist, max_dist of every clean, used point into
 *             record[mp_slot] and nothing else: desc, n_obs and bad keep their bits, and a dirty or unused point's record is not touched
 *             (the host sends those after its EraseObservation logic with dvm_map_store_update, as before).  The caller issues it under
 *             Map::mMutexMapUpdate, where Optimizer.cc:1357-1384 writes back.  The next optimize on the handle waits (on its stream) for
 *             a queued commit before it overwrites what that commit reads.  The map stores must outlive the commit.
 *   DVM_ERR_STATE: commit before any optimize, after an optimize that failed, of a window committed already (k = -1 with nothing left
 *             is DVM_OK), of a window whose ref_edge was NULL; k outside [-1, K) is DVM_ERR_INVALID.
 *   Refused on the host before anything is queued, no output written, the handle and a previous optimize's commits left as they were
 *   except that a refused optimize counts as failed: DVM_ERR_INVALID -- a NULL array, a store on another device, a keyframe slot outside
 *             its store, never written or removed, an edge index out of range, kp outside [0, n) of its slot, a map slot out of range,
 *             never written or named twice in one window, ref_edge[l] out of range or not an edge of point l (-1 is legal only on a
 *             point without edges), an invalid model; DVM_ERR_CAPACITY -- more than 30 free cameras in a window.
 *   last_bytes  what the last optimize sent up (tables, observations, slot lists, views) and fetched.
 * Calls on one handle are not concurrent; the calls on the stores it names follow the stores' rules.  sizeof(dvm_ba_obs) == 12,
 * sizeof(dvm_ba_window_resident) == 192 (LP64). */
typedef struct { int32_t pose, point, kp; } dvm_ba_obs;   /* camera and point of THIS window, keypoint index in that camera's keyframe */
typedef struct {
  int32_t n_poses, n_points, n_edges, iterations;
  const double* poses;           /* [n_poses][7] world -> camera, as dvm_ba_window */
  const uint8_t* fixed;          /* [n_poses] */
  const dvm_keyframe_store* keyframes;
  const int32_t* kf_slot;        /* [n_poses] */
  const float* ow;               /* [n_poses][3] or NULL: GetCameraCenter() of the FIXED cameras (rows of free cameras are not read) */
  dvm_map_store* points;
  const int32_t* mp_slot;        /* [n_points], each slot at most once per window */
  const dvm_ba_obs* obs;         /* [n_edges], a point's edges in MapPoint::GetObservations() order */
  const int32_t* ref_edge;       /* [n_points] or NULL: the edge that is the point's observation by mpRefKF; NULL: the window cannot be committed */
  dvm_ba_camera cam;             /* as dvm_ba_window (huber_delta read for every model) */
  double chi2_erase;             /* 5.991 for the monocular edge */
  double* poses_out;             /* as dvm_ba_window, any may be NULL */
  double* points_out;
  double* edge_chi2_out;
  uint8_t* depth_positive_out;
  float* geometry_out;           /* [n_points][8] or NULL: pos[3], normal[3], min_dist, max_dist as the commit would write them */
  uint8_t* point_dirty_out;      /* [n_points] or NULL */
  float* ow_out;                 /* [n_poses][3] or NULL: the camera centres the normals were taken from */
} dvm_ba_window_resident;
typedef struct dvm_ba_resident dvm_ba_resident;
int dvm_ba_resident_create(int device, dvm_ba_resident** out);
void dvm_ba_resident_destroy(dvm_ba_resident* h);
int dvm_ba_resident_optimize(dvm_ba_resident* h, const dvm_ba_window_resident* windows, const dvm_camera_model* models /* [K] or NULL: pinhole cam */,
                             int K, const volatile uint8_t* stop_flag, dvm_ba_stats* stats);
int dvm_ba_resident_commit(dvm_ba_resident* h, int k /* window of the last optimize; -1: every window not yet committed */);
int dvm_ba_resident_last_bytes(const dvm_ba_resident* h, int64_t* host_to_device, int64_t* device_to_host);

/* ---- Rows beside the keyframes: which map point does keypoint kp of the keyframe in slot j hold.  Two int32 rows per keyframe-store
 * slot, each as long as the slot's n, their values slots of a dvm_map_store:
 *   DVM_KFS_ROW_MATCHES   GetMapPointMatches() as map-store slots, -1 for a NULL pointer (UpdateLocalPoints reads it).
 *   DVM_KFS_ROW_OBSERVED  entry kp = the slot of the map point whose mObservations holds (this keyframe, kp), -1 otherwise: the inverse
 *                         of GetObservations() (the votes of UpdateLocalKeyFrames read it).
 * The two differ in the reference: a keyframe Tracking::CreateNewKeyFrame has queued has its mvpMapPoints set, and its points get their
 * AddObservation only in LocalMapping::ProcessNewKeyFrame.  Until then it is walked by UpdateLocalPoints and receives no votes.
 * The rows live in an allocation of their own -- capacity x (slot_keypoints rounded up to 16) x 4 B per kind, plus 4 B per slot for the
 * row's length on the device -- made by the first call that sets a row of that kind: a store on which no row call is made behaves and
 * allocates as before, and the slot layout (csrc/kf_store_layout.h) and every view of a slot are untouched.
 *   set_rows    rows[k] (the slot's n entries) becomes slot slots[k]'s row of kind `which`.
 *   patch_rows  edits[i] = {slot, kp, value}: the mirror of AddObservation / EraseObservation (OBSERVED) and AddMapPoint /
 *               EraseMapPointMatch / ReplaceMapPointMatch (MATCHES); MapPoint::Replace is both.  The edits of one call apply in order: the
 *               last edit of a cell wins (the host collapses duplicates before anything is queued; no two threads write one cell).  A
 *               slot whose row is not set opens as n entries of -1 first.
 *   points      the map store the values name.  Every value is checked on the host at set or patch time: -1 or a written slot of
 *               `points`.  The store remembers per slot and kind which map store its row names; a map store's capacity is fixed and a
 *               written slot stays written, so a row checked once stays valid: no kernel indexes a store with a value the host has not
 *               checked, and no per-tick call re-checks a row.  `points` outlives the rows that name it.
 *   ordering    that of dvm_keyframe_store_put: page-locked staging, ONE copy and a scatter kernel (k_kfs_rows_set / k_kfs_rows_patch) per
 *               round on the STORE'S OWN STREAM; the call may return before the kernel has run, every later reader waits for it, and it
 *               never overtakes a reader in flight.
 *   unset       put, put_device, put_tracked and remove of a slot unset both of its rows (host state, and the slot's device length goes
 *               back to 0 on the store's stream): a new keyframe holds nothing until it is told.  The device keeps each slot's row
 *               length per kind -- 0 for a slot never set, unset or removed --, so a kernel walks a store without a host-made list.
 *   refusals    DVM_ERR_INVALID before anything is queued, each naming the offender, nothing written: a slot outside the store, never
 *               put or removed; a NULL row where the slot holds keypoints; kp outside [0, n); a value below -1, outside `points` or
 *               never written; a `points` on another device; a slot named twice in one set_rows; `which` unknown; a patch of a row that
 *               names another map store.
 *   debug_read_rows  one row back, synchronous (tests): *n_out = the row's length (0 for a row not set), out [cap] its entries;
 *               DVM_ERR_CAPACITY with *n_out set when cap is too small.
 *   dvm_keyframe_store_last_put_bytes also reports the row calls.
 * sizeof(dvm_kfs_row_edit) == 12. */
#define DVM_KFS_ROW_MATCHES  0
#define DVM_KFS_ROW_OBSERVED 1
typedef struct { int32_t slot, kp, value; } dvm_kfs_row_edit;      /* 12 B */
int dvm_keyframe_store_set_rows(dvm_keyframe_store* s, int which, const dvm_map_store* points, int n, const int32_t* slots,
                                const int32_t* const* rows);
int dvm_keyframe_store_patch_rows(dvm_keyframe_store* s, int which, const dvm_map_store* points, int n_edits, const dvm_kfs_row_edit* edits);
int dvm_keyframe_store_debug_read_rows(dvm_keyframe_store* s, int which, int slot, int32_t* out, int cap, int32_t* n_out);

/* ---- Tracking::UpdateLocalMap() on the resident stores (csrc/update_local_map.cpp): the two graph walks between the halves of a tracked
 * frame (reference src/Tracking.cc:3108-3274) as list intersections over the rows above.  Both calls serve the `count` frames of one tick;
 * each frame names its own keyframe store and map store (one agent each; frames may share stores).  Each call is ONE upload, ONE chain of
 * batched launches on the handle's stream and ONE synchronisation; the results come down through a mapped page-locked block.  A call is a
 * READER of every store it names: it sees every dvm_map_store_update / _refresh, dvm_ba_resident_commit, put and row edit queued before
 * it with no host synchronisation between, and none of those overtakes it.  What stays host work is :3207-3251: one neighbour, one child
 * and one parent per local keyframe and the choice of pKFmax -- index work on the votes.
 *   reserve     grow-only: `max_frames` frames of up to `max_frame_keypoints` keypoints and `max_local_keyframes` named keyframes, on map
 *               stores of up to `map_capacity` slots and keyframe stores of up to `kf_capacity` slots of `slot_keypoints`.  The handle
 *               holds three tables of map_capacity words per frame (mult, first, pos).  They are idle between calls: every call puts
 *               back the entries it touched; there is no capacity-sized memset per call.
 *   keyframes   the vote loop of UpdateLocalKeyFrames (:3145-3181).  in[b].mp_slot [n]: the frame's mvpMapPoints as map-store slots, -1
 *               for none (mCurrentFrame's list, or mLastFrame's in the branch of :3162; the caller chooses).
 *               out[b].votes [capacity of in[b].kfs]: votes[j] = sum over kp of mult[OBSERVED[j][kp]], mult[s] = the number of the
 *               frame's keypoints that hold the non-bad point s -- a point held twice votes twice, as the reference's loop does; 0 for a
 *               slot without an OBSERVED row.  out[b].frame_bad [n]: 1 where keypoint i names a record with bad != 0 -- the entries the
 *               reference sets to NULL at :3157 / :3177; they do not vote.
 *               Kernels: k_ulm_mult (integer atomicAdd per frame entry), k_ulm_votes (one wavefront per (frame, keyframe slot): 16-byte
 *               row loads, mult gathered, a wave reduction, one word written), k_ulm_mult_reset.
 *               Upload: 64 * count + sum over frames of 4 * ceil16(n_b) bytes (ceil16: rounded up to a multiple of 16 entries, 64 B).
 *   points      UpdateLocalPoints (:3117-3141) plus the frame_mp of dvm_local_map_in_resident.  in[b].kf_slot [n_kfs]: mvpLocalKeyFrames
 *               in the order the loop visits them (the vector reversed); in[b].mp_slot [n]: the frame's list after the clearing above.
 *               The entries are the named slots' MATCHES rows numbered flat in (keyframe, keypoint) order; an entry is taken iff its
 *               value is >= 0, its record is not bad and no earlier entry names the same slot.  out[b].local_slot [local_cap]: the taken
 *               entries in flat order -- mvpLocalMapPoints as slots, in the reference's order; n_local their count.  out[b].frame_mp [n]:
 *               the position in local_slot of the point keypoint i holds; -1 where it holds none, the point is bad, or the point is in
 *               no named row -- n_outside counts the last case (the second half's precondition is that it is 0; the caller decides).
 *               n_local > local_cap: DVM_ERR_CAPACITY, n_local holds the full count, nothing is written past local_slot[local_cap) and
 *               frame_mp and n_outside are complete for every frame of the call.
 *               Kernels: k_ulm_mark (integer atomicMin of the key k * padded row length + kp), k_ulm_count / k_ulm_scan / k_ulm_write
 *               (stable compaction; the write records pos[slot]), k_ulm_frame_mp, k_ulm_points_reset.
 *               Upload: 64 * count + sum over frames of 4 * (ceil16(n_b) + ceil16(n_kfs_b)) bytes.  No row travels.
 *   refusals    on the host before anything is queued, each naming frame and entry; the handle stays usable and its tables idle.
 *               DVM_ERR_INVALID: a NULL argument with a non-zero count; a store on another device; a frame slot below -1, outside its
 *               map store or never written; a kf_slot outside the store, never put, removed or without a MATCHES row; a kf_slot named
 *               twice in one frame; a named row -- for the votes: any OBSERVED row of the store -- that names another map store than
 *               in[b].points.  DVM_ERR_CAPACITY: anything beyond the reservation.  Legal: count = 0, n = 0, n_kfs = 0, a row of length
 *               0, every entry -1, every point bad.
 *   failures    a HIP error behind a call's first launch (DVM_ERR_HIP): the outputs are not valid, the stores' read brackets are closed
 *               (a later writer waits for whatever the handle's stream still holds), and the next call on the handle writes the three
 *               tables idle again before it runs -- a failed call never leaves entries that a later call would count.
 *   last_bytes  the last call's one upload, and what was copied out of the mapped block.
 *   profile / last_ms  with profiling on, the kernels' time of the last call by HIP events (measurement only).
 * local_slot and frame_mp are what dvm_local_map_in_resident::slots and frame_mp take.  Calls on one handle are not concurrent.
 * sizeof(dvm_ulm_keyframes_in) == 32 (kfs 0, points 8, n 16, mp_slot 24); sizeof(dvm_ulm_keyframes_out) == 16 (votes 0, frame_bad 8);
 * sizeof(dvm_ulm_points_in) == 48 (kfs 0, points 8, n_kfs 16, kf_slot 24, n 32, mp_slot 40); sizeof(dvm_ulm_points_out) == 32
 * (local_slot 0, local_cap 8, n_local 12, frame_mp 16, n_outside 24) (LP64). */
typedef struct {
  const dvm_keyframe_store* kfs; const dvm_map_store* points;
  int32_t n; const int32_t* mp_slot;               /* [n] the frame's mvpMapPoints as slots of `points`, -1: none */
} dvm_ulm_keyframes_in;
typedef struct {
  int32_t* votes;                                  /* [dvm_keyframe_store_capacity(kfs)] */
  uint8_t* frame_bad;                              /* [n] */
} dvm_ulm_keyframes_out;
typedef struct {
  const dvm_keyframe_store* kfs; const dvm_map_store* points;
  int32_t n_kfs; const int32_t* kf_slot;           /* [n_kfs] mvpLocalKeyFrames as keyframe-store slots, in the loop's order */
  int32_t n; const int32_t* mp_slot;               /* [n] the frame's list, bad entries cleared or not (they count as none) */
} dvm_ulm_points_in;
typedef struct {
  int32_t* local_slot; int32_t local_cap;          /* [local_cap] */
  int32_t n_local;                                 /* written: the full count */
  int32_t* frame_mp;                               /* [n] */
  int32_t n_outside;                               /* written */
} dvm_ulm_points_out;
typedef struct dvm_update_local_map dvm_update_local_map;
int dvm_update_local_map_create(int device, dvm_update_local_map** out);
void dvm_update_local_map_destroy(dvm_update_local_map* h);
int dvm_update_local_map_reserve(dvm_update_local_map* h, int max_frames, int max_frame_keypoints, int max_local_keyframes, int map_capacity,
                                 int kf_capacity, int slot_keypoints);
int dvm_update_local_map_keyframes(dvm_update_local_map* h, int count, const dvm_ulm_keyframes_in* in, const dvm_ulm_keyframes_out* out);
int dvm_update_local_map_points(dvm_update_local_map* h, int count, const dvm_ulm_points_in* in, dvm_ulm_points_out* out);
int dvm_update_local_map_last_bytes(const dvm_update_local_map* h, int64_t* host_to_device, int64_t* device_to_host);
int dvm_update_local_map_profile(dvm_update_local_map* h, int enable);
int dvm_update_local_map_last_ms(const dvm_update_local_map* h, float* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif
