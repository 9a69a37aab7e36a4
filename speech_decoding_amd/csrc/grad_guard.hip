// The gradient guard: sum of squares and non-finite count of ALL parameter gradients (one launch over sda_adam_multi's
// descriptor table), and the step's decision — skip on inf / NaN, loss-scale update, clip coefficient, bias corrections — taken
// by one workgroup into a device state vector.  sda_adam_multi_guarded (param_ops.hip) reads that vector; the host never does.
// Everything is double; the summation order is fixed, so the bits depend on the gradients alone.
#include <math.h>

#include "sd_common.h"

namespace sda {

// inf and NaN: all exponent bits set (a comparison could be folded away under a fast-math build; the bit test cannot)
__device__ inline void guard_add(double& s, unsigned& bad, float g) {
  if ((__float_as_uint(g) & 0x7f800000u) == 0x7f800000u) ++bad;
  else s += (double)g * (double)g;             // fp32 x fp32 is exact in double
}

// Fixed tree over the 256 threads of the workgroup; the total lands in thread 0's (s, c).
__device__ inline void guard_tree(double& s, double& c, double (*sh)[256]) {
  const int t = threadIdx.x;
  sh[0][t] = s;
  sh[1][t] = c;
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) {
      sh[0][t] += sh[0][t + off];
      sh[1][t] += sh[1][t + off];
    }
    __syncthreads();
  }
  s = sh[0][0];
  c = sh[1][0];
}

// Grid (gx, n) as adam_multi_kernel: workgroup (b, t) reads the elements of tensor t that Adam's workgroup (b, t) updates.
__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(const sda_adam_desc* __restrict__ descs, double* __restrict__ partials) {
  __shared__ double sh[2][256];
  const sda_adam_desc d = descs[blockIdx.y];
  double s = 0.0;
  unsigned bad = 0;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < d.n; i += (long)gridDim.x * 1024) {
    if (i + 4 <= d.n && d.aligned) {
      const float4 g = *reinterpret_cast<const float4*>(d.grad + i);
      guard_add(s, bad, g.x);
      guard_add(s, bad, g.y);
      guard_add(s, bad, g.z);
      guard_add(s, bad, g.w);
    } else {
      for (long j = i; j < min(i + 4, d.n); ++j) guard_add(s, bad, d.grad[j]);
    }
  }
  double c = (double)bad;
  guard_tree(s, c, sh);
  if (threadIdx.x == 0) {
    double* o = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = s;
    o[1] = c;
  }
}

__global__ __launch_bounds__(256) void grad_guard_finish_kernel(const double* __restrict__ partials, long slots, double* __restrict__ state,
                                                                double max_norm, float beta1, float beta2, double growth_interval,
                                                                double max_scale, int dynamic) {
  __shared__ double sh[2][256];
  double s = 0.0, c = 0.0;
  for (long k = threadIdx.x; k < slots; k += 256) {
    s += partials[2 * k];
    c += partials[2 * k + 1];
  }
  guard_tree(s, c, sh);
  if (threadIdx.x != 0) return;
  const double scale = state[SDA_GUARD_SCALE];
  state[SDA_GUARD_SUMSQ] = s;
  state[SDA_GUARD_NONFINITE] = c;
  if (c > 0.0) {
    state[SDA_GUARD_SKIP] = 1.0;
    state[SDA_GUARD_SKIPPED] += 1.0;
    state[SDA_GUARD_GOOD] = 0.0;
    state[SDA_GUARD_NORM] = HUGE_VAL;
    state[SDA_GUARD_COEF] = 0.0;
    if (dynamic) state[SDA_GUARD_SCALE] = fmax(1.0, scale * 0.5);
    return;
  }
  const double step = state[SDA_GUARD_STEP] + 1.0;
  double good = state[SDA_GUARD_GOOD] + 1.0;
  if (dynamic && good >= growth_interval) {
    state[SDA_GUARD_SCALE] = fmin(max_scale, 2.0 * scale);
    good = 0.0;
  }
  const double norm = sqrt(s) / scale;
  double clip = 1.0;
  if (max_norm > 0.0 && max_norm < HUGE_VAL) clip = fmin(1.0, max_norm / (norm + 1e-6));
  state[SDA_GUARD_SKIP] = 0.0;
  state[SDA_GUARD_STEP] = step;
  state[SDA_GUARD_GOOD] = good;
  state[SDA_GUARD_NORM] = norm;
  state[SDA_GUARD_COEF] = (1.0 / scale) * clip;
  state[SDA_GUARD_BC1] = (double)(float)(1.0 - pow((double)beta1, step));
  state[SDA_GUARD_BC2_SQRT] = (double)(float)sqrt(1.0 - pow((double)beta2, step));
}

static inline long guard_gx(long max_n) {
  const long gx = (max_n + 1023) / 1024;
  return gx > 256 ? 256 : gx;
}

}  // namespace sda

using namespace sda;

extern "C" long sda_grad_guard_parts(int n, long max_n) {
  if (n < 1 || max_n < 1) { set_error("grad_guard_parts: n or max_n < 1"); return -1; }
  return 2L * n * guard_gx(max_n);
}

extern "C" int sda_grad_sumsq_multi(const sda_adam_desc* descs_dev, int n, long max_n, double* partials, void* stream) {
  if (!descs_dev || !partials || n < 1 || max_n < 1) { set_error("grad_sumsq_multi: bad arguments (null pointer, n or max_n < 1)"); return -1; }
  hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3((unsigned)guard_gx(max_n), (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     descs_dev, partials);
  return check_launch("grad_sumsq_multi");
}

extern "C" int sda_grad_guard_finish(const double* partials, int n, int gx, double* state, double max_norm, float beta1, float beta2,
                                     long growth_interval, double max_scale, int dynamic, void* stream) {
  if (!partials || !state) { set_error("grad_guard_finish: null pointer"); return -1; }
  if (n < 1 || gx < 1 || growth_interval < 0 || max_norm != max_norm || !(max_scale >= 1.0)) {
    set_error("grad_guard_finish: bad arguments (n or gx < 1, growth_interval < 0, NaN max_norm or max_scale < 1)");
    return -1;
  }
  hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long)n * gx, state, max_norm,
                     beta1, beta2, (double)growth_interval, max_scale, dynamic);
  return check_launch("grad_guard_finish");
}
