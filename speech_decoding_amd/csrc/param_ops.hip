// Parameter-side passes: conv weights and per-channel vectors into their padded (and GLU-split) operand layouts, weight
// gradients back out of them with the ordered sum over the K-split slabs, and Adam.  All fp32 except the packed operands.
#include <math.h>

#include "sd_common.h"

namespace sda {

// ------------------------------------------------------------------------------------------------
// weight / vector packing
// ------------------------------------------------------------------------------------------------
__device__ inline int glu_unmap(int cop, int Cout, int half, int half_p, int tile = 0) {   // packed row -> source row or -1
  if (half == 0) return cop < Cout ? cop : -1;
  if (tile > 0) {                        // SDA_EPI_GLU layout: per 2*tile packed channels, `tile` values then `tile` gates
    const int j = cop / (2 * tile), w = cop - j * 2 * tile;
    const int r = j * tile + (w < tile ? w : w - tile);          // channel inside its half
    if (w < tile) return r < half ? r : -1;
    return r < Cout - half ? half + r : -1;
  }
  if (cop < half_p) return cop < half ? cop : -1;
  const int r = cop - half_p;
  return r < Cout - half ? half + r : -1;
}
__device__ inline int glu_map(int co, int half, int half_p) { return (half == 0 || co < half) ? co : half_p + co - half; }

// Value of element i of a packed conv weight, 0 in the padding.  mode 0: [n][tap][co'][ci'] (forward operand); mode 1:
// [n][KS - 1 - tap][ci'][co'] (data-gradient operand: taps reversed, channels swapped).  Source: w[n][co][ci][tap].
__device__ inline float packed_weight_value(const float* __restrict__ w, size_t i, int Cout, int Cin, int KS, int Cout_p,
                                            int Cin_p, int mode, int half, int half_p, int tile) {
  int co, ci, tap;
  size_t q = i;
  if (mode == 0) {
    ci = q % Cin_p; q /= Cin_p;
    co = glu_unmap((int)(q % Cout_p), Cout, half, half_p, tile); q /= Cout_p;
    tap = q % KS; q /= KS;
  } else {
    co = glu_unmap((int)(q % Cout_p), Cout, half, half_p, tile); q /= Cout_p;
    ci = q % Cin_p; q /= Cin_p;
    tap = KS - 1 - (int)(q % KS); q /= KS;
  }
  const int n = (int)q;
  float v = 0.f;
  if (co >= 0 && ci < Cin) v = w[(((size_t)n * Cout + co) * Cin + ci) * KS + tap];
  return v;
}

template <typename E>
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, E* __restrict__ dst, int nW, int Cout, int Cin,
                                        int KS, int Cout_p, int Cin_p, int mode, int half, int half_p) {
  const size_t total = (size_t)nW * KS * Cout_p * Cin_p;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    Elem<E>::st(dst + i, packed_weight_value(w, i, Cout, Cin, KS, Cout_p, Cin_p, mode, half, half_p, 0));
}

__global__ void unpack_conv_wgrad_kernel(const float* __restrict__ g, float* __restrict__ dst, int nW, int Cout,
                                         int Cin, int KS, int Cout_p, int Cin_p, int half, int half_p) {
  const size_t total = (size_t)nW * Cout * Cin * KS;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    size_t q = i;
    const int tap = q % KS; q /= KS;
    const int ci = q % Cin; q /= Cin;
    const int co = q % Cout; q /= Cout;
    const int n = (int)q;
    dst[i] = g[(((size_t)n * KS + tap) * Cout_p + glu_map(co, half, half_p)) * Cin_p + ci];
  }
}

// All operand packs of one step in ONE launch: blockIdx.y selects the descriptor (device array).
template <typename E>
__global__ void pack_multi_kernel(const sda_pack_desc* __restrict__ descs) {
  const sda_pack_desc d = descs[blockIdx.y];
  const size_t total = (size_t)d.total;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    if (d.is_vector) {
      const int c = glu_unmap((int)i, d.Cout, d.glu_half, d.glu_half_p, d.glu_tile);
      reinterpret_cast<float*>(d.dst)[i] = c >= 0 ? d.src[c] : 0.f;
      continue;
    }
    Elem<E>::st(reinterpret_cast<E*>(d.dst) + i,
                packed_weight_value(d.src, i, d.Cout, d.Cin, d.KS, d.Cout_p, d.Cin_p, d.mode, d.glu_half, d.glu_half_p, d.glu_tile));
  }
}

// Sum over the K-split slabs of the V (float or float4) at slabs[k * slab + src], k = 0 .. nslabs - 1: 8 independent loads in
// flight, then added in slab order, the tail one at a time — the sum order does not depend on the batching, and it decides the
// bits of every weight gradient.
__device__ inline void slab_add(float& s, float v) { s += v; }
__device__ inline void slab_add(float4& s, const float4& v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }

template <typename V>
__device__ inline V ordered_slab_sum(const float* __restrict__ slabs, int nslabs, size_t slab, size_t src) {
  V sum = {};
  int k = 0;
  for (; k + 8 <= nslabs; k += 8) {
    V v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const V*>(slabs + (size_t)(k + j) * slab + src);
#pragma unroll
    for (int j = 0; j < 8; ++j) slab_add(sum, v[j]);
  }
  for (; k < nslabs; ++k) slab_add(sum, *reinterpret_cast<const V*>(slabs + (size_t)k * slab + src));
  return sum;
}

// dst[co][ci][tap] = sum_s slabs[s][tap][co'][ci]   (ordered sum over the K-split slabs + un-packing in one pass)
__global__ void reduce_unpack_wgrad_kernel(const float* __restrict__ slabs, int nslabs, float* __restrict__ dst, int Cout,
                                           int Cin, int KS, int Cout_p, int Cin_p, int half, int half_p) {
  const size_t total = (size_t)Cout * Cin * KS;
  const size_t slab = (size_t)KS * Cout_p * Cin_p;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    // thread order follows the SOURCE layout ([tap][co][ci], ci fastest) so the slab reads coalesce
    size_t q = i;
    const int ci = q % Cin; q /= Cin;
    const int co = q % Cout; q /= Cout;
    const int tap = (int)q;
    const size_t src = ((size_t)tap * Cout_p + glu_map(co, half, half_p)) * Cin_p + ci;
    dst[((size_t)co * Cin + ci) * KS + tap] = ordered_slab_sum<float>(slabs, nslabs, slab, src);
  }
}

// The same on 16-byte loads (Cin % 4 == 0, slabs 16-byte aligned): a thread sums FOUR consecutive input channels of one
// (tap, co) — a quarter of the threads, each with 8 x 16 B in flight; identical sums (each output adds its slabs in slab order)
__global__ __launch_bounds__(256) void reduce_unpack_wgrad_vec_kernel(const float* __restrict__ slabs, int nslabs, float* __restrict__ dst,
                                                                      int Cout, int Cin, int KS, int Cout_p, int Cin_p, int half, int half_p) {
  const int cin4 = Cin >> 2;
  const size_t total = (size_t)Cout * cin4 * KS;
  const size_t slab = (size_t)KS * Cout_p * Cin_p;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    size_t q = i;
    const int c4 = q % cin4; q /= cin4;
    const int co = q % Cout; q /= Cout;
    const int tap = (int)q;
    const size_t src = ((size_t)tap * Cout_p + glu_map(co, half, half_p)) * Cin_p + 4 * c4;
    const float4 sum = ordered_slab_sum<float4>(slabs, nslabs, slab, src);
    float* o = dst + ((size_t)co * Cin + 4 * c4) * KS + tap;
    o[0] = sum.x; o[KS] = sum.y; o[2 * KS] = sum.z; o[3 * KS] = sum.w;
  }
}

__global__ void reduce_slabs_kernel(const float* __restrict__ src, float* __restrict__ dst, int nslabs, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dst[i] = ordered_slab_sum<float>(src, nslabs, (size_t)n, (size_t)i);
}

__global__ void pack_vector_kernel(const float* __restrict__ v, float* __restrict__ dst, int C, int Cp, int half, int half_p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Cp) return;
  const int c = glu_unmap(i, C, half, half_p);
  dst[i] = c >= 0 ? v[c] : 0.f;
}
__global__ void unpack_vector_kernel(const float* __restrict__ g, float* __restrict__ dst, int C, int half, int half_p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) dst[i] = g[glu_map(i, half, half_p)];
}

static inline int ew_grid(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace sda

using namespace sda;

extern "C" int sda_pack_conv_weight(const float* w, void* dst, int nW, int Cout, int Cin, int KS, int Cout_p,
                                    int Cin_p, int mode, int glu_half, int glu_half_p, int dtype, void* stream) {
  if (!w || !dst || nW < 1 || Cout > Cout_p || Cin > Cin_p || (mode != 0 && mode != 1)) { set_error("pack_conv_weight: bad arguments"); return -1; }
  if (glu_half && (glu_half_p < glu_half || glu_half_p + (Cout - glu_half) > Cout_p)) { set_error("pack_conv_weight: bad GLU split"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)nW * KS * Cout_p * Cin_p;
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(pack_conv_weight_kernel<E>, dim3(ew_grid(total)), dim3(256), 0, st, w,
                                         (E*)dst, nW, Cout, Cin, KS, Cout_p, Cin_p, mode, glu_half, glu_half_p));
  return check_launch("pack_conv_weight");
}

extern "C" int sda_unpack_conv_wgrad(const float* g, float* dst, int nW, int Cout, int Cin, int KS, int Cout_p,
                                     int Cin_p, int glu_half, int glu_half_p, void* stream) {
  if (!g || !dst) { set_error("unpack_conv_wgrad: null"); return -1; }
  const size_t total = (size_t)nW * Cout * Cin * KS;
  hipLaunchKernelGGL(unpack_conv_wgrad_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, g, dst, nW,
                     Cout, Cin, KS, Cout_p, Cin_p, glu_half, glu_half_p);
  return check_launch("unpack_conv_wgrad");
}

// Adam (train.py:161-163: torch.optim.Adam defaults, no weight decay / amsgrad) over ALL parameter tensors in
// one launch: blockIdx.y selects the tensor, complex parameters are updated through their real view.
// adam_multi_body is the update of both kernels below, so that they compile the same arithmetic: COEF = false is
// sda_adam_multi's (the gradient as stored), COEF = true sda_adam_multi_guarded's (the gradient times `coef`, rounded to fp32
// by a multiply of its own — __fmul_rn is never contracted into the sums behind it).
template <bool COEF>
__device__ __forceinline__ void adam_multi_body(const sda_adam_desc& d, float lr, float beta1, float beta2, float eps, float bc1,
                                                float bc2_sqrt, float coef) {
  const float step_size = lr / bc1;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < d.n; i += (long)gridDim.x * 1024) {
    if (i + 4 <= d.n && d.aligned) {
      float4 p = *reinterpret_cast<float4*>(d.param + i);
      float4 g = *reinterpret_cast<const float4*>(d.grad + i);
      if (COEF) { g.x = __fmul_rn(g.x, coef); g.y = __fmul_rn(g.y, coef); g.z = __fmul_rn(g.z, coef); g.w = __fmul_rn(g.w, coef); }
      float4 m = *reinterpret_cast<float4*>(d.exp_avg + i), v = *reinterpret_cast<float4*>(d.exp_avg_sq + i);
#define SDA_ADAM(f)                                                     \
      m.f = beta1 * m.f + (1.f - beta1) * g.f;                          \
      v.f = beta2 * v.f + (1.f - beta2) * g.f * g.f;                    \
      p.f -= step_size * (m.f / (sqrtf(v.f) / bc2_sqrt + eps));
      SDA_ADAM(x) SDA_ADAM(y) SDA_ADAM(z) SDA_ADAM(w)
#undef SDA_ADAM
      *reinterpret_cast<float4*>(d.param + i) = p;
      *reinterpret_cast<float4*>(d.exp_avg + i) = m;
      *reinterpret_cast<float4*>(d.exp_avg_sq + i) = v;
    } else {
      for (long j = i; j < min(i + 4, d.n); ++j) {
        const float g = COEF ? __fmul_rn(d.grad[j], coef) : d.grad[j];
        const float m = beta1 * d.exp_avg[j] + (1.f - beta1) * g;
        const float v = beta2 * d.exp_avg_sq[j] + (1.f - beta2) * g * g;
        d.exp_avg[j] = m;
        d.exp_avg_sq[j] = v;
        d.param[j] -= step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
      }
    }
  }
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const sda_adam_desc* __restrict__ descs, float lr, float beta1,
                                                         float beta2, float eps, float bc1, float bc2_sqrt) {
  const sda_adam_desc d = descs[blockIdx.y];
  adam_multi_body<false>(d, lr, beta1, beta2, eps, bc1, bc2_sqrt, 1.f);
}

// The same update behind the gradient guard (grad_guard.hip): the step is decided on the device.  state[SDA_GUARD_SKIP] set:
// every thread returns before its first load, nothing is written.  Otherwise the gradient is multiplied by
// (float)state[SDA_GUARD_COEF] (un-scaling and clipping in one factor) and both bias corrections are the ones
// sda_grad_guard_finish left in `state` for the step it counted.
__global__ __launch_bounds__(256) void adam_multi_guarded_kernel(const sda_adam_desc* __restrict__ descs, float lr, float beta1,
                                                                 float beta2, float eps, const double* __restrict__ state) {
  if (state[SDA_GUARD_SKIP] != 0.0) return;
  const sda_adam_desc d = descs[blockIdx.y];
  adam_multi_body<true>(d, lr, beta1, beta2, eps, (float)state[SDA_GUARD_BC1], (float)state[SDA_GUARD_BC2_SQRT],
                        (float)state[SDA_GUARD_COEF]);
}

extern "C" int sda_adam_multi(const sda_adam_desc* descs_dev, int n, long max_n, float lr, float beta1, float beta2, float eps,
                              long step, void* stream) {
  if (!descs_dev || n < 1 || max_n < 1 || step < 1) { set_error("adam_multi: bad arguments"); return -1; }
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long gx = (max_n + 1023) / 1024;
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, descs_dev, lr, beta1,
                     beta2, eps, (float)bc1, (float)sqrt(bc2));
  return check_launch("adam_multi");
}

extern "C" int sda_adam_multi_guarded(const sda_adam_desc* descs_dev, int n, long max_n, float lr, float beta1, float beta2,
                                      float eps, const double* state, void* stream) {
  if (!descs_dev || !state || n < 1 || max_n < 1) { set_error("adam_multi_guarded: bad arguments (null pointer, n or max_n < 1)"); return -1; }
  long gx = (max_n + 1023) / 1024;
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(adam_multi_guarded_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, descs_dev, lr,
                     beta1, beta2, eps, state);
  return check_launch("adam_multi_guarded");
}

extern "C" int sda_pack_multi(const sda_pack_desc* descs_dev, int n, long max_total, int dtype, void* stream) {
  if (!descs_dev || n < 1 || max_total < 1) { set_error("pack_multi: bad arguments"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  long gx = (max_total + 1023) / 1024;
  if (gx > 512) gx = 512;
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(pack_multi_kernel<E>, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, st, descs_dev));
  return check_launch("pack_multi");
}

extern "C" int sda_reduce_unpack_wgrad(const float* slabs, int nslabs, float* dst, int Cout, int Cin, int KS, int Cout_p,
                                       int Cin_p, int glu_half, int glu_half_p, void* stream) {
  if (!slabs || !dst || nslabs < 1) { set_error("reduce_unpack_wgrad: bad arguments"); return -1; }
  const size_t total = (size_t)Cout * Cin * KS;
  if (Cin % 4 == 0 && Cin_p % 4 == 0 && (reinterpret_cast<uintptr_t>(slabs) & 15) == 0) {
    hipLaunchKernelGGL(reduce_unpack_wgrad_vec_kernel, dim3(ew_grid(total / 4)), dim3(256), 0, (hipStream_t)stream, slabs, nslabs, dst,
                       Cout, Cin, KS, Cout_p, Cin_p, glu_half, glu_half_p);
    return check_launch("reduce_unpack_wgrad");
  }
  hipLaunchKernelGGL(reduce_unpack_wgrad_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, slabs, nslabs, dst,
                     Cout, Cin, KS, Cout_p, Cin_p, glu_half, glu_half_p);
  return check_launch("reduce_unpack_wgrad");
}

extern "C" int sda_reduce_slabs(const float* src, float* dst, int nslabs, long n, void* stream) {
  if (!src || !dst || nslabs < 1 || n < 1) { set_error("reduce_slabs: bad arguments"); return -1; }
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3(ew_grid((size_t)n)), dim3(256), 0, (hipStream_t)stream, src, dst, nslabs, n);
  return check_launch("reduce_slabs");
}

extern "C" int sda_pack_vector(const float* v, float* dst, int C, int Cp, int glu_half, int glu_half_p, void* stream) {
  if (!v || !dst || C > Cp) { set_error("pack_vector: bad arguments"); return -1; }
  hipLaunchKernelGGL(pack_vector_kernel, dim3((Cp + 255) / 256), dim3(256), 0, (hipStream_t)stream, v, dst, C, Cp,
                     glu_half, glu_half_p);
  return check_launch("pack_vector");
}

extern "C" int sda_unpack_vector(const float* g, float* dst, int C, int Cp, int glu_half, int glu_half_p, void* stream) {
  if (!g || !dst || C > Cp) { set_error("unpack_vector: bad arguments"); return -1; }
  hipLaunchKernelGGL(unpack_vector_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, dst, C,
                     glu_half, glu_half_p);
  return check_launch("unpack_vector");
}
