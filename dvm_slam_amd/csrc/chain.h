// dvm_slam_amd/csrc/chain.h -- what the "one device chain" entry points share (track.cpp, new_points.cpp, fuse_targets.cpp): the device
// check of every entry point of the library, a reserved working set (a device block plus a page-locked twin), the cursor that packs an
// upload and carves results at equal offsets of both, a handle's stream life cycle and its optional HIP-event kernel times.  A new chain
// is its kernels, its pack and its unpack on top of these.  Plain structs and inline functions; the byte layouts stay with the callers
// (each passes its own alignment and its own order of items).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>

#include "orb_pipeline.h"   // set_error / hip_check / DVM_HIP

namespace dvm {

// ---- the device check.  need_any_device(): some HIP device is visible, for the entry points that take no device index (they run on the
// calling thread's current device and do not select one).  need_device(device): that, the index in range, and the device selected.
inline int need_any_device(int* count = nullptr) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_error("no HIP device visible (libdvmslam_hip has no CPU path)");
    return DVM_ERR_NO_DEVICE;
  }
  if (count) *count = n;
  return DVM_OK;
}
inline int need_device(int device) {
  int n = 0;
  const int rc = need_any_device(&n);
  if (rc != DVM_OK) return rc;
  if (device < 0 || device >= n) {
    set_error("device index out of range");
    return DVM_ERR_INVALID;
  }
  return hip_check(hipSetDevice(device), "hipSetDevice");
}

// ---- two copies of one block at equal offsets
template <size_t A> constexpr size_t pad(size_t b) { return (b + A - 1) & ~(A - 1); }
// where the copy at `to` holds what p is in the copy at `from`
template <class T> T* rebase(T* p, const uint8_t* from, uint8_t* to) { return reinterpret_cast<T*>(to + (reinterpret_cast<const uint8_t*>(p) - from)); }

// the memory of one reservation: a device block and a page-locked block, each beginning with the upload region (built in the page-locked
// block, copied to the same offsets of the device block by one asynchronous copy)
struct WorkingSet {
  uint8_t* d = nullptr;                           // device
  uint8_t *hm = nullptr, *hm_dev = nullptr;       // page-locked: host address; its device address when mapped
  size_t up_bytes = 0;                            // the upload region's capacity
  // replaces what it holds by dbytes of device memory and hbytes of page-locked memory, the first `up` bytes of each the upload region -- mapped into the device's address space (kernels
  // write results to it) or plain (an explicit copy back) -- zeroed or as it comes; on failure it holds nothing and names what failed
  const char* alloc(size_t dbytes, size_t hbytes, size_t up, bool mapped, bool zeroed) {
    free();
    if (hipMalloc(reinterpret_cast<void**>(&d), dbytes) != hipSuccess) { d = nullptr; return "hipMalloc"; }
    if (hipHostMalloc(reinterpret_cast<void**>(&hm), hbytes, mapped ? hipHostMallocMapped : hipHostMallocDefault) != hipSuccess) {
      hm = nullptr; free();
      return mapped ? "mapped host memory" : "page-locked host memory";
    }
    if (mapped && hipHostGetDevicePointer(reinterpret_cast<void**>(&hm_dev), hm, 0) != hipSuccess) { free(); return "mapped host memory"; }
    if (zeroed) std::memset(hm, 0, hbytes);
    up_bytes = up;
    return nullptr;
  }
  void free() {
    if (d) hipFree(d);
    if (hm) hipHostFree(hm);
    d = hm = hm_dev = nullptr; up_bytes = 0;
  }
  template <class T> T* dev(T* host_ptr) const { return rebase(host_ptr, hm, hm_dev); }
};

// walks a block and its twin at equal offsets, every item rounded up to A bytes: carve reserves an item in `base`, put copies one into
// `base` and returns where the twin holds it (staging block -> device block).  On a null base carve only measures: it advances off and
// returns null (no address is formed), so a layout is written once and used() of it at the largest arguments is the size to reserve.
template <size_t A> struct Cursor {
  uint8_t* base;
  uint8_t* twin = nullptr;
  size_t off = 0;
  template <class T> T* carve(size_t count) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += pad<A>(count * sizeof(T));
    return r;
  }
  uint8_t* put(const void* src, size_t bytes) {
    uint8_t* r = twin + off;
    if (bytes) std::memcpy(base + off, src, bytes);
    off += pad<A>(bytes);
    return r;
  }
  size_t used() const { return off; }             // bytes so far: the one upload's length, and what the one overflow check compares
};

// kernel times of a chain: up to kMarks events recorded between its launches, when enabled
struct EventTimer {
  static constexpr int kMarks = 4;
  hipEvent_t ev[kMarks] = {};
  bool on = false;
  int enable(bool e) {
    if (e)
      for (hipEvent_t& x : ev) if (!x) DVM_HIP(hipEventCreate(&x));
    on = e;
    return DVM_OK;
  }
  hipError_t mark(int i, hipStream_t s) const { return on ? hipEventRecord(ev[i], s) : hipSuccess; }
  hipError_t elapsed(int i, int j, float* ms) const { return hipEventElapsedTime(ms, ev[i], ev[j]); }
  void destroy() { for (hipEvent_t& x : ev) if (x) { hipEventDestroy(x); x = nullptr; } }
};

// the part every chain handle begins with (struct dvm_xxx : dvm::Chain)
struct Chain {
  int device = 0;
  hipStream_t s = nullptr;
  WorkingSet ws;
  EventTimer timer;
};
// dvm_xxx_create: device check -> the handle -> its non-blocking stream
template <class H> int chain_create(int device, H** out) {
  if (!out) return DVM_ERR_INVALID;
  *out = nullptr;
  int rc = need_device(device);
  if (rc != DVM_OK) return rc;
  H* h = new (std::nothrow) H;
  if (!h) return DVM_ERR_INVALID;
  h->device = device;
  rc = hip_check(hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking), "hipStreamCreate");
  if (rc != DVM_OK) { delete h; return rc; }
  *out = h;
  return DVM_OK;
}
// dvm_xxx_destroy: what is queued runs out, then the stream, the events and the working set go
template <class H> void chain_destroy(H* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->s) { hipStreamSynchronize(h->s); hipStreamDestroy(h->s); }
  h->timer.destroy();
  h->ws.free();
  delete h;
}

}  // namespace dvm
