// tools/check_track_settle.cpp -- the per-frame epilogue of the tracked-frame host calls (dvm_slam_amd/host/track_settle.h) on hand-written
// frames: a complete frame with one outlier, a frame below 20 matches, a frame with no assignment at all, and the resident id source.  Every
// expected value is written out here.  Plain g++, no device library (tests/test_host_logic.py builds it, also with sanitizers).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../dvm_slam_amd/host/track_settle.h"

using dvm_host::HostIds;
using dvm_host::SlotIds;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

template <class T, size_t N> static bool eq(const std::vector<T>& got, const T (&want)[N]) {
  return got.size() == N && std::memcmp(got.data(), want, N * sizeof(T)) == 0;
}

static dvm_se3f pred() { return dvm_se3f{{0.1f, -0.2f, 0.3f, 0.9f}, {1.5f, -2.5f, 3.5f}}; }

int main() {
  // LastFrame: keypoints 0..6 hold map points 40, -1, 42, 43, -1, 45, 46; queries were built from keypoints 0, 2, 3, 5, 6
  const int32_t mp_l[7] = {40, -1, 42, 43, -1, 45, 46};
  const int qi[5] = {0, 2, 3, 5, 6};
  const HostIds host_ids{mp_l, qi};
  {   // a complete frame of 6 keypoints: 4 matched, the match of keypoint 3 rejected by PoseOptimization
    dvm_track_result r{};
    r.n = 6; r.mono_index = 5; r.status = DVM_TRACK_COMPLETE; r.nmatches = 4; r.n_edges = 4; r.n_inliers = 3; r.nmatches_map = 2; r.nmatches_after = 3;
    r.n_requeried = 7;
    const double pose[7] = {0.1, 0.2, 1.0 / 3.0, 1e-9, -0.5, 0.25, 0.8125000001};
    std::memcpy(r.pose, pose, sizeof pose);
    const int32_t assign[6] = {4, -1, 0, 2, -1, 1};
    const uint8_t outlier[6] = {0, 1, 0, 1, 0, 0};      // (the flag of the unmatched keypoint 1 is not read)
    std::vector<int32_t> mp_c(6, 99), dropped(6, 99);
    dvmh_track_result out{};
    dvm_host::settle_tracked_frame(r, assign, outlier, host_ids, pred(), 1, mp_c.data(), dropped.data(), &out);
    const int32_t want_mp[6] = {46, -1, 40, -1, -1, 42}, want_dr[6] = {-1, -1, -1, 43, -1, -1};
    EXPECT(eq(mp_c, want_mp)); EXPECT(eq(dropped, want_dr));
    EXPECT(out.n == 6 && out.mono_index == 5 && out.nmatches == 3 && out.nmatches_search == 4 && out.nmatches_map == 2 && out.n_inliers == 3);
    EXPECT(out.wide_window == 1 && out.replayed_on_host == 0 && out.tracked == 1 && out.n_requeried == 7);
    EXPECT(std::memcmp(out.pose, pose, sizeof pose) == 0);
    const float want_t[3] = {(float)0.1, (float)0.2, (float)(1.0 / 3.0)}, want_q[4] = {(float)1e-9, -0.5f, 0.25f, (float)0.8125000001};
    EXPECT(std::memcmp(out.Tcw.t, want_t, 12) == 0 && std::memcmp(out.Tcw.q, want_q, 16) == 0);
    EXPECT(out.Tcw.q[3] == 0.8125f);                     // the double rounds to the float, it is not truncated or kept
  }
  {   // fewer than 20 matches, 5 keypoints: the search's matches stay, nothing dropped, the pose is the prediction
    dvm_track_result r{};
    r.n = 5; r.mono_index = 5; r.status = DVM_TRACK_FEW_MATCHES; r.nmatches = 2; r.n_requeried = 1;
    r.nmatches_after = 77; r.nmatches_map = 77; r.n_inliers = 77;      // (not read for such a frame)
    const int32_t assign[5] = {-1, 3, -1, -1, 1};
    const uint8_t outlier[5] = {1, 1, 1, 1, 1};          // (not read either)
    std::vector<int32_t> mp_c(5, 99), dropped(5, 99);
    dvmh_track_result out{};
    const dvm_se3f T = pred();
    dvm_host::settle_tracked_frame(r, assign, outlier, host_ids, T, 1, mp_c.data(), dropped.data(), &out);
    const int32_t want_mp[5] = {-1, 45, -1, -1, 42}, want_dr[5] = {-1, -1, -1, -1, -1};
    EXPECT(eq(mp_c, want_mp)); EXPECT(eq(dropped, want_dr));
    EXPECT(out.n == 5 && out.nmatches == 2 && out.nmatches_search == 2 && out.nmatches_map == 0 && out.n_inliers == 0 && out.tracked == 0);
    EXPECT(out.wide_window == 1 && out.n_requeried == 1);
    EXPECT(std::memcmp(&out.Tcw, &T, sizeof T) == 0);
    const double want_pose[7] = {(double)1.5f, (double)-2.5f, (double)3.5f, (double)0.1f, (double)-0.2f, (double)0.3f, (double)0.9f};
    EXPECT(std::memcmp(out.pose, want_pose, sizeof want_pose) == 0);
  }
  {   // no assignment at all, 4 keypoints, no wide window (a frame whose LastFrame held no points: status FEW_MATCHES with 0 matches)
    dvm_track_result r{};
    r.n = 4; r.mono_index = 4; r.status = DVM_TRACK_FEW_MATCHES;
    const int32_t assign[4] = {-1, -1, -1, -1};
    const uint8_t outlier[4] = {0, 0, 0, 0};
    std::vector<int32_t> mp_c(6, 99), dropped(6, 99);   // two entries beyond n: left alone
    dvmh_track_result out{};
    dvm_host::settle_tracked_frame(r, assign, outlier, HostIds{nullptr, nullptr}, pred(), 0, mp_c.data(), dropped.data(), &out);
    const int32_t want[6] = {-1, -1, -1, -1, 99, 99};
    EXPECT(eq(mp_c, want)); EXPECT(eq(dropped, want));
    EXPECT(out.n == 4 && out.mono_index == 4 && out.nmatches == 0 && out.nmatches_search == 0 && out.tracked == 0 && out.wide_window == 0);
  }
  {   // the resident id source: queries numbered by entry, ids are the entry lists' slots; a complete frame of 4 keypoints, one outlier
    const int32_t slot[3] = {900, 17, 512};
    dvm_track_result r{};
    r.n = 4; r.mono_index = 4; r.status = DVM_TRACK_COMPLETE; r.nmatches = 3; r.n_inliers = 2; r.nmatches_map = 1; r.nmatches_after = 2;
    const double pose[7] = {-1.0, 2.0, -3.0, 0.0, 0.0, 0.0, 1.0};
    std::memcpy(r.pose, pose, sizeof pose);
    const int32_t assign[4] = {2, 0, -1, 1};
    const uint8_t outlier[4] = {0, 1, 0, 0};
    std::vector<int32_t> mp_c(4, 99), dropped(4, 99);
    dvmh_track_result out{};
    dvm_host::settle_tracked_frame(r, assign, outlier, SlotIds{slot}, pred(), 0, mp_c.data(), dropped.data(), &out);
    const int32_t want_mp[4] = {512, -1, -1, 17}, want_dr[4] = {-1, 900, -1, -1};
    EXPECT(eq(mp_c, want_mp)); EXPECT(eq(dropped, want_dr));
    EXPECT(out.nmatches == 2 && out.nmatches_search == 3 && out.nmatches_map == 1 && out.n_inliers == 2 && out.tracked == 1 && out.wide_window == 0);
    const float want_t[3] = {-1.0f, 2.0f, -3.0f}, want_q[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    EXPECT(std::memcmp(out.Tcw.t, want_t, 12) == 0 && std::memcmp(out.Tcw.q, want_q, 16) == 0 && std::memcmp(out.pose, pose, sizeof pose) == 0);
  }
  {   // the same status under the resident source when the chain hands a frame back unfinished (status 2): settled as not tracked
    const int32_t slot[2] = {8, 9};
    dvm_track_result r{};
    r.n = 4; r.status = DVM_TRACK_REPLAY_ON_HOST; r.nmatches = 30;
    const int32_t assign[4] = {1, -1, 0, -1};
    const uint8_t outlier[4] = {0, 0, 0, 0};
    std::vector<int32_t> mp_c(4, 99), dropped(4, 99);
    dvmh_track_result out{};
    dvm_host::settle_tracked_frame(r, assign, outlier, SlotIds{slot}, pred(), 0, mp_c.data(), dropped.data(), &out);
    const int32_t want_mp[4] = {9, -1, 8, -1}, want_dr[4] = {-1, -1, -1, -1};
    EXPECT(eq(mp_c, want_mp)); EXPECT(eq(dropped, want_dr));
    EXPECT(out.tracked == 0 && out.nmatches == 30 && out.nmatches_search == 30 && out.replayed_on_host == 0);
  }
  if (fails) return 1;
  std::printf("track settle: all frames as written\n");
  return 0;
}
