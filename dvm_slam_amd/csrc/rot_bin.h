// dvm_slam_amd/csrc/rot_bin.h -- the rotation-histogram bin of ORBmatcher (HISTO_LENGTH = 30, e.g. src/ORBmatcher.cc:324-329): the one
// float expression the host mirror (host/orb_matcher.cpp) and the device chains (track_kernels.hip) both evaluate.
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
}  // namespace dvm
