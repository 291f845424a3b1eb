// dvm_slam_amd/csrc/f64_spec.hip -- dvm_f64_spec_eval: csrc/f64_spec.h evaluated on the device (tests: the device build against the host
// build and the oracle's restatement, bit for bit)
#include <hip/hip_runtime.h>

#include "../../include/dvmslam_hip.h"
#include "f64_spec.h"
#include "host_stage.h"

namespace dvm {
__global__ void k_f64_spec(const double* __restrict__ x, int n, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = f64_sin(x[i]); out[n + i] = f64_cos(x[i]); out[2 * n + i] = f64_cube(x[i]);
}
}  // namespace dvm

using namespace dvm;

extern "C" int dvm_f64_spec_eval(int device, const double* x, int n, double* out) {
  if (n < 0 || (n && (!x || !out))) return DVM_ERR_INVALID;
  if (n == 0) return DVM_OK;
  int rc = dvm_set_device(device);
  if (rc != DVM_OK) return rc;
  Stage st;
  const int ix = st.in(x, 8 * (size_t)n), io = st.out(out, 24 * (size_t)n);
  if ((rc = st.upload()) != DVM_OK) return rc;
  hipLaunchKernelGGL(k_f64_spec, dim3((n + 255) / 256), dim3(256), 0, st.stream(), st.ptr<double>(ix), n, st.ptr<double>(io));
  DVM_HIP(hipGetLastError());
  return st.download();
}
