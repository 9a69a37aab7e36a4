// MSELoss (speech_decoding/utils/loss.py:15-25): loss = sum_{b,f,t} (Y - Z)^2 / b_div, dZ = 2 dloss (Z - Y) / b_div, dY = -dZ.
// Purely HBM-bound.  Each operand is either a row-layout buffer (channels-last, cp channels) or a plain contiguous (B, F, T)
// tensor, in fp32 / bf16 / fp16.  The work is cut into 64-channel x 64-step tiles of one sample; a thread owns 16-byte runs of
// Z in Z's own layout (along channels for row layout, along time for plain), so Z and dZ move with 16-byte accesses.  When Y
// has the other layout its tile is staged through LDS as fp32 [f][t] (read coalesced along its own contiguous axis), and a dY
// goes back out the same way.  Sums: fp32 per tile and thread, fp64 across tiles, one fp64 partial per workgroup of a grid
// whose size depends on the shape alone, then a fixed-order final sum in a second launch: no atomics, the same bits every call.
#include "sd_common.h"

namespace sda {
namespace {

constexpr int MSE_TF = 64;                  // channels per tile
constexpr int MSE_TT = 64;                  // time steps per tile
constexpr int MSE_LD = MSE_TT + 1;          // LDS pitch (floats) of a staged [f][t] tile: every access pattern below is conflict-free
constexpr int MSE_THREADS = 256;

struct MseDims {
  int B, F, T, zcp, ycp, nft, ntt, b_div;
  long ntiles;
  int pvec;                                 // plain operands take 16-byte runs along t (T % 8 == 0, 16-byte aligned pointers)
};

__device__ __forceinline__ size_t rows_off(int b, int t, int T, int cp, int f) { return ((size_t)b * rows_tp(T) + PAD + t) * cp + f; }
__device__ __forceinline__ size_t plain_off(int b, int f, int t, int F, int T) { return ((size_t)b * F + f) * T + t; }

// M consecutive elements <-> floats with the widest accesses M allows (16 bytes; 8 bytes for 4 16-bit elements)
template <typename E, int M> __device__ __forceinline__ void load_run(const E* p, float* v) {
  constexpr int V = Vec16<E>::N;
  if constexpr (M >= V) {
#pragma unroll
    for (int j = 0; j < M / V; ++j) Vec16<E>::load(p + j * V, v + j * V);
  } else {
    static_assert(M == 4, "runs are 4 or 8 elements");
    const float4 f = load4(p);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  }
}
template <typename E, int M> __device__ __forceinline__ void store_run(E* p, const float* v) {
  constexpr int V = Vec16<E>::N;
  if constexpr (M >= V) {
#pragma unroll
    for (int j = 0; j < M / V; ++j) Vec16<E>::store(p + j * V, v + j * V);
  } else {
    static_assert(M == 4, "runs are 4 or 8 elements");
    store4(p, make_float4(v[0], v[1], v[2], v[3]));
  }
}

// Y's tile -> stage[f][t], read in Y's own layout (positions outside the tensor are not written)
template <typename EY, bool YR>
__device__ __forceinline__ void stage_in(const EY* __restrict__ y, float* stage, int b, int f0, int t0, const MseDims& d) {
  constexpr int N = Vec16<EY>::N, CPR = (YR ? MSE_TF : MSE_TT) / N, ITEMS = MSE_TF * MSE_TT / N / MSE_THREADS;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int idx = threadIdx.x + i * MSE_THREADS;
    const int major = idx / CPR, minor = (idx % CPR) * N;
    float v[N];
    if constexpr (YR) {                                  // run along channels of row t0 + major
      if (t0 + major >= d.T) continue;
      load_run<EY, N>(y + rows_off(b, t0 + major, d.T, d.ycp, f0 + minor), v);
#pragma unroll
      for (int k = 0; k < N; ++k) stage[(minor + k) * MSE_LD + major] = v[k];
    } else {                                             // run along time of channel f0 + major
      const int f = f0 + major, t = t0 + minor;
      if (f >= d.F || t >= d.T) continue;
      const EY* p = y + plain_off(b, f, t, d.F, d.T);
      if (d.pvec) {
        load_run<EY, N>(p, v);
#pragma unroll
        for (int k = 0; k < N; ++k) stage[major * MSE_LD + minor + k] = v[k];
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (t + k < d.T) stage[major * MSE_LD + minor + k] = Elem<EY>::ld(p + k);
      }
    }
  }
}

// stage[f][t] -> dY's tile in Y's layout; row layout: pad channels written as zeros
template <typename EY, bool YR>
__device__ __forceinline__ void stage_out(EY* __restrict__ dy, const float* stage, int b, int f0, int t0, const MseDims& d) {
  constexpr int N = Vec16<EY>::N, CPR = (YR ? MSE_TF : MSE_TT) / N, ITEMS = MSE_TF * MSE_TT / N / MSE_THREADS;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int idx = threadIdx.x + i * MSE_THREADS;
    const int major = idx / CPR, minor = (idx % CPR) * N;
    float v[N];
    if constexpr (YR) {
      if (t0 + major >= d.T) continue;
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] = f0 + minor + k < d.F ? stage[(minor + k) * MSE_LD + major] : 0.f;
      store_run<EY, N>(dy + rows_off(b, t0 + major, d.T, d.ycp, f0 + minor), v);
    } else {
      const int f = f0 + major, t = t0 + minor;
      if (f >= d.F || t >= d.T) continue;
      EY* p = dy + plain_off(b, f, t, d.F, d.T);
      if (d.pvec) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = stage[major * MSE_LD + minor + k];
        store_run<EY, N>(p, v);
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (t + k < d.T) Elem<EY>::st(p + k, stage[major * MSE_LD + minor + k]);
      }
    }
  }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ZR / YR: Z / Y in row layout.  Forward (BWD = false): partial[blockIdx.x] = this workgroup's sum of squares.
// Backward: dz (Z's form) = s (Z - Y), dy (Y's form, may be null) = -s (Z - Y), s = (dloss / b_div) * 2 as autograd forms it.
template <typename EZ, bool ZR, typename EY, bool YR, bool BWD>
__global__ __launch_bounds__(MSE_THREADS) void mse_kernel(const EZ* __restrict__ z, const EY* __restrict__ y, EZ* __restrict__ dz,
                                                          EY* __restrict__ dy, const float* __restrict__ dloss,
                                                          double* __restrict__ partial, const MseDims d) {
  constexpr bool STAGE = ZR != YR;
  constexpr int NZ = Vec16<EZ>::N, CPR = (ZR ? MSE_TF : MSE_TT) / NZ, ITEMS = MSE_TF * MSE_TT / NZ / MSE_THREADS;
  __shared__ float stage[STAGE ? MSE_TF * MSE_LD : 1];
  __shared__ double red[MSE_THREADS / 64];
  float s = 0.f;
  if constexpr (BWD) s = (dloss[0] / (float)d.b_div) * 2.0f;
  double acc = 0.0;
  for (long tile = blockIdx.x; tile < d.ntiles; tile += gridDim.x) {
    const int ft = (int)(tile % d.nft);
    const long r = tile / d.nft;
    const int tt = (int)(r % d.ntt), b = (int)(r / d.ntt);
    const int f0 = ft * MSE_TF, t0 = tt * MSE_TT;
    if constexpr (STAGE) {
      __syncthreads();                               // the previous tile's readers and dY writers are done with `stage`
      stage_in<EY, YR>(y, stage, b, f0, t0, d);
      __syncthreads();
    }
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int idx = threadIdx.x + i * MSE_THREADS;
      const int major = idx / CPR, minor = (idx % CPR) * NZ;
      const int fi = ZR ? minor : major, ti = ZR ? major : minor;      // tile position of the run's first element
      const int f = f0 + fi, t = t0 + ti;
      // element k of the run is (f + k, t) in row layout, (f, t + k) in plain layout
      if (t >= d.T || (!ZR && f >= d.F)) continue;
      const bool vec = ZR || d.pvec;                 // the whole run lies inside the tensor and moves as vectors
      const size_t zo = ZR ? rows_off(b, t, d.T, d.zcp, f) : plain_off(b, f, t, d.F, d.T);
      const size_t yo = YR ? rows_off(b, t, d.T, d.ycp, f) : plain_off(b, f, t, d.F, d.T);   // (same layout as Z only)
      bool ok[NZ];
      float zv[NZ], yv[NZ], g[NZ];
#pragma unroll
      for (int k = 0; k < NZ; ++k) ok[k] = ZR ? f + k < d.F : (vec || t + k < d.T);
      if (vec) {
        load_run<EZ, NZ>(z + zo, zv);
      } else {
#pragma unroll
        for (int k = 0; k < NZ; ++k) zv[k] = ok[k] ? Elem<EZ>::ld(z + zo + k) : 0.f;
      }
      if constexpr (STAGE) {
#pragma unroll
        for (int k = 0; k < NZ; ++k) yv[k] = stage[ZR ? (fi + k) * MSE_LD + ti : fi * MSE_LD + ti + k];
      } else if (vec) {
        load_run<EY, NZ>(y + yo, yv);
      } else {
#pragma unroll
        for (int k = 0; k < NZ; ++k) yv[k] = ok[k] ? Elem<EY>::ld(y + yo + k) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < NZ; ++k) {
        const float dd = ok[k] ? zv[k] - yv[k] : 0.f;   // (a select: stale LDS / pad values never reach the sum)
        if constexpr (BWD) g[k] = ok[k] ? s * dd : 0.f;
        else part = __builtin_fmaf(dd, dd, part);
      }
      if constexpr (BWD) {
        if (dz) {
          if (vec) {
            store_run<EZ, NZ>(dz + zo, g);
          } else {
#pragma unroll
            for (int k = 0; k < NZ; ++k)
              if (ok[k]) Elem<EZ>::st(dz + zo + k, g[k]);
          }
        }
        if (dy) {
#pragma unroll
          for (int k = 0; k < NZ; ++k) g[k] = ok[k] ? -g[k] : 0.f;      // (pad channels: +0, not -0)
          if constexpr (STAGE) {
#pragma unroll
            for (int k = 0; k < NZ; ++k)
              if (ZR || ok[k]) stage[ZR ? (fi + k) * MSE_LD + ti : fi * MSE_LD + ti + k] = g[k];
          } else if (vec) {
            store_run<EY, NZ>(dy + yo, g);
          } else {
#pragma unroll
            for (int k = 0; k < NZ; ++k)
              if (ok[k]) Elem<EY>::st(dy + yo + k, g[k]);
          }
        }
      }
    }
    if constexpr (BWD && STAGE) {
      if (dy) {
        __syncthreads();
        stage_out<EY, YR>(dy, stage, b, f0, t0, d);
      }
    }
    if constexpr (!BWD) acc += (double)part;
  }
  if constexpr (!BWD) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// loss[0] = (sum of the n partials, fixed order) / b_div
__global__ __launch_bounds__(256) void mse_final_kernel(const double* __restrict__ partial, int n, int b_div, float* __restrict__ loss) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {                      // fixed tree: deterministic
    if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(sh[0] / (double)b_div);
}

template <typename EZ, typename EY, bool BWD>
void launch_mse(bool zr, bool yr, int grid, const void* z, const void* y, void* dz, void* dy, const float* dloss, double* partial,
                const MseDims& d, hipStream_t st) {
  const EZ* zp = (const EZ*)z;
  const EY* yp = (const EY*)y;
  EZ* dzp = (EZ*)dz;
  EY* dyp = (EY*)dy;
#define SDA_MSE_LAUNCH(ZR, YR) \
  hipLaunchKernelGGL((mse_kernel<EZ, ZR, EY, YR, BWD>), dim3(grid), dim3(MSE_THREADS), 0, st, zp, yp, dzp, dyp, dloss, partial, d)
  if (zr && yr) SDA_MSE_LAUNCH(true, true);
  else if (zr) SDA_MSE_LAUNCH(true, false);
  else if (yr) SDA_MSE_LAUNCH(false, true);
  else SDA_MSE_LAUNCH(false, false);
#undef SDA_MSE_LAUNCH
}

template <bool BWD>
int dispatch_mse(int zt, int yt, bool zr, bool yr, int grid, const void* z, const void* y, void* dz, void* dy, const float* dloss,
                 double* partial, const MseDims& d, hipStream_t st) {
#define SDA_MSE_Y(EZ)                                                                                        \
  switch (yt) {                                                                                              \
    case SDA_F32: launch_mse<EZ, float, BWD>(zr, yr, grid, z, y, dz, dy, dloss, partial, d, st); break;     \
    case SDA_BF16: launch_mse<EZ, uint16_t, BWD>(zr, yr, grid, z, y, dz, dy, dloss, partial, d, st); break;  \
    default: launch_mse<EZ, half_t, BWD>(zr, yr, grid, z, y, dz, dy, dloss, partial, d, st); break;          \
  }
  switch (zt) {
    case SDA_F32: SDA_MSE_Y(float) break;
    case SDA_BF16: SDA_MSE_Y(uint16_t) break;
    default: SDA_MSE_Y(half_t) break;
  }
#undef SDA_MSE_Y
  return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// shared argument checks; fills d and the grid.  Returns 0 or -1 (message set).
int mse_setup(const char* what, const void* z, int z_cp, int z_dtype, const void* y, int y_cp, int y_dtype, int B, int F, int T,
              int b_div, const void* dz, const void* dy, MseDims& d, int& grid) {
  if (!z || !y) { set_error("%s: null operand", what); return -1; }
  if (B < 1 || F < 1 || T < 1 || b_div < 1) { set_error("%s: bad sizes (B %d, F %d, T %d, b_div %d)", what, B, F, T, b_div); return -1; }
  const int dts[2] = {z_dtype, y_dtype}, cps[2] = {z_cp, y_cp};
  for (int i = 0; i < 2; ++i) {
    if (dts[i] != SDA_F32 && dts[i] != SDA_BF16 && dts[i] != SDA_F16) { set_error("%s: unknown dtype %d", what, dts[i]); return -1; }
    if (cps[i] < 0 || (cps[i] > 0 && (cps[i] % SDA_CH_ALIGN || cps[i] < F))) {
      set_error("%s: a row-layout operand needs a channel pitch that is a multiple of %d and >= F (got %d, F %d)", what, SDA_CH_ALIGN, cps[i], F);
      return -1;
    }
  }
  if (z_cp > 0 && y_cp > 0 && z_cp != y_cp) { set_error("%s: row-layout operands of different channel pitch (%d, %d)", what, z_cp, y_cp); return -1; }
  const void* zs[2] = {z, dz};
  const void* ys[2] = {y, dy};
  bool plain_aligned = true;
  for (int i = 0; i < 2; ++i) {
    if (z_cp > 0 && zs[i] && !aligned16(zs[i])) { set_error("%s: row-layout buffers must be 16-byte aligned", what); return -1; }
    if (y_cp > 0 && ys[i] && !aligned16(ys[i])) { set_error("%s: row-layout buffers must be 16-byte aligned", what); return -1; }
    if (z_cp == 0 && zs[i] && !aligned16(zs[i])) plain_aligned = false;
    if (y_cp == 0 && ys[i] && !aligned16(ys[i])) plain_aligned = false;
  }
  d.B = B; d.F = F; d.T = T; d.zcp = z_cp; d.ycp = y_cp; d.b_div = b_div;
  d.nft = ((z_cp > 0 ? z_cp : F) + MSE_TF - 1) / MSE_TF;     // row-layout Z: every channel tile, so dZ's pad channels get their zeros
  d.ntt = (T + MSE_TT - 1) / MSE_TT;
  d.ntiles = (long)B * d.ntt * d.nft;
  d.pvec = (T % 8 == 0) && plain_aligned;
  grid = (int)(d.ntiles < SDA_MSE_PARTIALS ? d.ntiles : SDA_MSE_PARTIALS);
  return 0;
}

}  // namespace
}  // namespace sda

extern "C" int sda_mse_forward(const void* z, int z_cp, int z_dtype, const void* y, int y_cp, int y_dtype, int B, int F, int T,
                               int b_div, double* scratch, float* loss, void* stream) {
  using namespace sda;
  MseDims d;
  int grid = 0;
  if (mse_setup("mse_forward", z, z_cp, z_dtype, y, y_cp, y_dtype, B, F, T, b_div, nullptr, nullptr, d, grid)) return -1;
  if (!scratch || !loss) { set_error("mse_forward: null scratch or loss"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  dispatch_mse<false>(z_dtype, y_dtype, z_cp > 0, y_cp > 0, grid, z, y, nullptr, nullptr, nullptr, scratch, d, st);
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, st, (const double*)scratch, grid, b_div, loss);
  return check_launch("mse_forward");
}

extern "C" int sda_mse_backward(const void* z, int z_cp, int z_dtype, const void* y, int y_cp, int y_dtype, int B, int F, int T,
                                int b_div, const float* dloss, void* dz, void* dy, void* stream) {
  using namespace sda;
  MseDims d;
  int grid = 0;
  if (mse_setup("mse_backward", z, z_cp, z_dtype, y, y_cp, y_dtype, B, F, T, b_div, dz, dy, d, grid)) return -1;
  if (!dloss || (!dz && !dy)) { set_error("mse_backward: null dloss, or neither dz nor dy"); return -1; }
  dispatch_mse<true>(z_dtype, y_dtype, z_cp > 0, y_cp > 0, grid, z, y, dz, dy, dloss, nullptr, d, (hipStream_t)stream);
  return check_launch("mse_backward");
}
