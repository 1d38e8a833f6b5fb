// Support-polygon math probe (test infrastructure, not the product): erf_f64 and exp_neg_sq of
// quadruped_control_amd/csrc/qc_device.hpp, one value per thread over arrays, so tests/test_gpu_support_polygon.py can hold the two
// primitives against a 50-digit reference.  The wrappers call the header's functions as they are; nothing here restates them.
// Every launcher takes device pointers (torch tensors), n and a stream and returns the hipError_t of its launch; qcs_breakpoints
// hands out the constants at which the two functions change form.
// Built by __graft_entry__.build_support_polygon_probe() with the product's own HIP_FLAGS (contraction and inlining as in the library).
#include "../../quadruped_control_amd/csrc/qc_device.hpp"

using namespace qc;

namespace {
constexpr int kBlock = 64;
inline dim3 grid_for(int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

__global__ void k_erf(const double* x, double* y, int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) y[i] = erf_f64(x[i]);
}
__global__ void k_exp_neg_sq(const double* x, double* y, int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) y[i] = exp_neg_sq(x[i]);
}
}  // namespace

extern "C" {
int qcs_erf(const double* x, double* y, int n, void* stream) {
  if (n <= 0) return 0;
  k_erf<<<grid_for(n), dim3(kBlock), 0, (hipStream_t)stream>>>(x, y, n);
  return (int)hipGetLastError();
}
int qcs_exp_neg_sq(const double* x, double* y, int n, void* stream) {
  if (n <= 0) return 0;
  k_exp_neg_sq<<<grid_for(n), dim3(kBlock), 0, (hipStream_t)stream>>>(x, y, n);
  return (int)hipGetLastError();
}
// out[0..3]: the |x| at which erf_f64 changes form (ERF_B0, ERF_B1, ERF_B2, ERF_ONE); out[4]: the a^2 from which exp_neg_sq is 0
void qcs_breakpoints(double* out) {
  out[0] = ERF_B0; out[1] = ERF_B1; out[2] = ERF_B2; out[3] = ERF_ONE; out[4] = EXP_NEG_SQ_ZERO;
}
}
