// dvm_slam_amd/csrc/rot_bin.h -- the rotation-histogram bin of ORBmatcher (HISTO_LENGTH = 30, e.g. src/ORBmatcher.cc:324-329): the one
// float expression the host mirror (host/orb_matcher.cpp) and the device chains (track_kernels.hip, new_points_kernels.hip) both evaluate,
// and ComputeThreeMaxima with the test it ends in, as the device chains run them.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DVM_ROT_HD __host__ __device__
#else
#define DVM_ROT_HD
#endif

namespace dvm {
constexpr int kRotHisto = 30;
// rot = a1 - a2 wrapped into [0, 360), bin = round(rot / 30) with 30 -> 0 (float arithmetic throughout: factor = 1.0f / 30)
DVM_ROT_HD inline int rot_bin(float a1, float a2) {
  const float factor = 1.0f / (float)kRotHisto;
  float rot = a1 - a2;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * factor);
  if (bin == kRotHisto) bin = 0;
  return bin;
}
// ComputeThreeMaxima (ORBmatcher.cc:1750-1802) over the bin counts: the three fullest bins, the second and third dropped below a
// tenth of the first (on the device: one lane)
DVM_ROT_HD inline void three_maxima(const int* hist, int* ind) {
  int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
  for (int i = 0; i < kRotHisto; i++) {
    const int sv = hist[i];
    if (sv > max1) { max3 = max2; max2 = max1; max1 = sv; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (sv > max2) { max3 = max2; max2 = sv; ind3 = ind2; ind2 = i; }
    else if (sv > max3) { max3 = sv; ind3 = i; }
  }
  if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
  ind[0] = ind1; ind[1] = ind2; ind[2] = ind3;
}
// the rotation check takes back a match whose bin is none of the three maxima (e.g. ORBmatcher.cc:1730-1745)
DVM_ROT_HD inline bool rot_dropped(int bin, const int* ind) { return bin != ind[0] && bin != ind[1] && bin != ind[2]; }
}  // namespace dvm
