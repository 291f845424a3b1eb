// dvm_slam_amd/host/chain_handle.h -- the calling thread's handle of a device chain (dvm_new_points, dvm_fuse_targets, dvm_bow_targets): created on first
// use, dropped and created again when the device changes, reserved on growth only -- never per call.  The caller decides what to reserve
// (its own headroom, its own pre-checks) and how to report a status that is not DVM_OK.
#pragma once
#include "dvmslam_hip.h"

namespace dvm_host {
template <class H, int (*Create)(int, H**), void (*Destroy)(H*), int (*Reserve)(H*, int, int, int)>
struct ChainHandle {
  H* h = nullptr;
  int device = -1;
  int cap[3] = {0, 0, 0};          // what is reserved, in the order of Reserve's arguments
  ChainHandle() = default;
  ChainHandle(const ChainHandle&) = delete;
  ChainHandle& operator=(const ChainHandle&) = delete;
  ~ChainHandle() { if (h) Destroy(h); }
  // the handle on device `dev`
  int open(int dev) {
    if (h && device != dev) { Destroy(h); h = nullptr; cap[0] = cap[1] = cap[2] = 0; }
    if (h) return DVM_OK;
    const int rc = Create(dev, &h);
    if (rc != DVM_OK) { h = nullptr; return rc; }
    device = dev;
    return DVM_OK;
  }
  bool holds(long a, long b, long c) const { return a <= cap[0] && b <= cap[1] && c <= cap[2]; }
  int reserve(int a, int b, int c) {
    const int rc = Reserve(h, a, b, c);
    if (rc == DVM_OK) { cap[0] = a; cap[1] = b; cap[2] = c; }
    return rc;
  }
};
}  // namespace dvm_host
