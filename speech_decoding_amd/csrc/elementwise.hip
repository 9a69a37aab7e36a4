// HBM-bound stages of the path over row-layout activations: BatchNorm statistics/apply (+GELU), GLU, GELU backward, column
// sums and per-sample sums of squares.  All kernels touch VALID rows only (pad rows stay zero) and move 16 bytes per lane
// (4 fp32 or 8 bf16 / fp16 channels).  Reductions are two-stage and ordered, so results are bitwise reproducible run to run.
// The row layout's own pack / unpack / fills are in row_layout.hip; weight and gradient packing, slab sums and Adam in param_ops.hip.
#include <math.h>

#include "sd_common.h"

namespace sda {

// ------------------------------------------------------------------------------------------------
// Row streaming skeleton of the elementwise passes.  A thread OWNS one 16-byte channel chunk (its per-channel
// coefficients stay in registers) and walks the valid rows of its workgroup's contiguous row range with stride RG =
// 256 / chunks-per-row; (sample, time) advance incrementally, so the loop has no integer division and no
// coefficient loads — with both, the BatchNorm/GELU passes were VALU-bound (≈ 4.3 TB/s), not HBM-bound.
// Rows are taken U at a time: all loads of a batch are issued before the first use.
// ------------------------------------------------------------------------------------------------
// Wave priority of the backward's HBM-bound passes on the step's main chain (BatchNorm backward, GLU / GELU backward with their
// column sums and the small reductions behind them): they run beside the weight-gradient GEMMs of the other stream, and at
// s_setprio 3 their loads and stores win the SIMD's issue arbitration against those waves.  Round 5, six alternations on
// one box (ms per step): off 6.771, on 6.777; with the data-gradient convs' waves raised as well (SDA_CONV_WAVE_PRIO) 6.725
// against 6.754 for those alone — the pair is worth 0.05 ms, either one alone nothing.
__device__ __forceinline__ void ew_bwd_prio() { __builtin_amdgcn_s_setprio(3); }

struct RowWalk {
  int r, r1, step, T, b, t;
  __device__ RowWalk(int r0, int r1_, int step_, int T_) : r(r0), r1(r1_), step(step_), T(T_) {
    b = r0 / T_;
    t = r0 - b * T_;
  }
  __device__ bool valid() const { return r < r1; }
  __device__ size_t mem_row() const { return (size_t)b * rows_tp(T) + PAD + t; }
  __device__ void next() {
    r += step; t += step;
    while (t >= T) { t -= T; ++b; }
  }
};

// The same walk reduced to what the inner loop needs: a 32-bit ELEMENT offset that advances by a constant and takes the
// pad rows in one extra add when the time index wraps (row-layout buffers stay below 2^32 elements: the launchers check),
// and the number of rows this thread owns — so the loop body has no validity predicates and no 64-bit multiplies.
struct RowCursor {
  uint32_t off, step, wrap;
  int t, T, RG, n;
  __device__ RowCursor(int r0, int r1, int rg, int RG_, int T_, int Cp, int col) : T(T_), RG(RG_) {
    const int first = r0 + rg;
    n = first < r1 ? (r1 - first + RG_ - 1) / RG_ : 0;
    const int b = first / T_;
    t = first - b * T_;
    off = (uint32_t)(b * rows_tp(T_) + PAD + t) * (uint32_t)Cp + (uint32_t)col;
    step = (uint32_t)RG_ * (uint32_t)Cp;
    wrap = (uint32_t)PAD * (uint32_t)Cp;
  }
  __device__ uint32_t take() {              // offset of the current row; moves to the next one
    const uint32_t o = off;
    off += step; t += RG;
    while (t >= T) { t -= T; off += wrap; }
    return o;
  }
};

// valid-row range of this workgroup: rows split evenly over the grid
__device__ inline void block_rows(int B, int T, int& r0, int& r1) {
  const int rows = B * T;
  const int per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
  r0 = min(rows, (int)blockIdx.x * per);
  r1 = min(rows, r0 + per);
}

// grid of a streaming pass: about 32 rows per thread-row group, at most 8 workgroups per CU
// RowCursor's offsets are 32-bit element indices
static inline bool fits_u32(int B, int T, long width) { return (unsigned long long)rows_alloc(B, T) * (unsigned long long)width < (1ull << 32); }

static inline int stream_blocks(int B, int T, int nch) {
  const long rows = (long)B * T;
  const int RG = nch >= 256 ? 1 : 256 / nch;
  long nb = (rows + (long)RG * 8 - 1) / ((long)RG * 8);
  return (int)(nb < 1 ? 1 : (nb > 2048 ? 2048 : nb));
}

// The five streaming kernels below each open with the same chunk loop (block_rows, RG, c over RG * nch), and three of them walk
// their RowCursor U rows at a time with a tail loop.  Both are spelled out per kernel on purpose: inside a shared helper taking
// the body as a lambda, the 16-bit bn_gelu_bwd_apply_kernel needs 94 VGPRs instead of 86 and its pass over a bf16
// (256, 320, 360) buffer takes 36.7 us instead of 35.3.

// ------------------------------------------------------------------------------------------------
// per-sample sum of squares (loss.py:64-65 norms), two-stage
// ------------------------------------------------------------------------------------------------
constexpr int SUMSQ_CHUNKS = 64;

template <typename E>
__global__ __launch_bounds__(256) void rows_sumsq_kernel(const E* __restrict__ x, float* __restrict__ scratch,
                                                         long row_elems, long pitch) {
  __shared__ float red[4];
  const int b = blockIdx.y, ch = blockIdx.x;
  const long n4 = row_elems / 4;
  const long per = (n4 + SUMSQ_CHUNKS - 1) / SUMSQ_CHUNKS;
  const long beg = ch * per, end = min(n4, beg + per);
  const E* p = x + (size_t)b * pitch;
  float s = 0.f;
  for (long i = beg + threadIdx.x; i < end; i += 256) {
    const float4 v = load4(p + i * 4);
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) scratch[b * SUMSQ_CHUNKS + ch] = red[0] + red[1] + red[2] + red[3];
}

__global__ void rows_sumsq_final_kernel(const float* __restrict__ scratch, float* __restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < SUMSQ_CHUNKS; ++i) s += (double)scratch[b * SUMSQ_CHUNKS + i];
  out[b] = (float)s;
}

// sum of s over the 256 threads of a workgroup in a fixed tree (deterministic); the result is thread 0's
__device__ inline double block_tree_sum(double s) {
  __shared__ double sh[256];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// per-sample sum of squares from the per-tile channel statistics a conv epilogue already wrote
// (stats[tile][1][c] = sum over the tile's valid rows of y^2): out[b] = sum over the sample's tiles and all channels
__global__ __launch_bounds__(256) void rows_sumsq_from_stats_kernel(const float* __restrict__ stats, int tiles_per_sample,
                                                                    int Cp, float* __restrict__ out) {
  const int b = blockIdx.x;
  double s = 0.0;
  for (int t = 0; t < tiles_per_sample; ++t) {
    const float* p = stats + (((size_t)b * tiles_per_sample + t) * 2 + 1) * Cp;
    for (int c = threadIdx.x; c < Cp; c += 256) s += (double)p[c];
  }
  s = block_tree_sum(s);
  if (threadIdx.x == 0) out[b] = (float)s;
}

// per-sample norms from conv1_flat's SDA_EPI_ROW_SUMSQ partials ([buffer row][n_parts]): sample b = rows b * (T + PAD) + PAD + t
__global__ __launch_bounds__(256) void rows_sumsq_from_row_parts_kernel(const float* __restrict__ parts, int n_parts, int T,
                                                                        float* __restrict__ out) {
  const int b = blockIdx.x;
  const float* p = parts + ((size_t)b * rows_tp(T) + PAD) * n_parts;
  double s = 0.0;
  for (int i = threadIdx.x; i < T * n_parts; i += 256) s += (double)p[i];
  s = block_tree_sum(s);
  if (threadIdx.x == 0) out[b] = (float)s;
}

// ------------------------------------------------------------------------------------------------
// BatchNorm1d: finalize / apply+GELU / backward   (models.py:135,143,158,161)
// ------------------------------------------------------------------------------------------------
// Sum partial[k][which][c] over k for the 8 channels of this block: 128 thread groups (2 lanes x float4
// each) stride over k, fp64 accumulation, fixed combination order (deterministic).  Result: channel
// 8*blockIdx.x + threadIdx.x on threads 0..7.
__device__ inline void block_partial_sums(const float* __restrict__ partial, int n, int Cp, int cbase, bool two,
                                          double& s0, double& s1) {
  // LDS image [which][j][thread]: every store and every load below is 64 consecutive 8-byte slots per wave (the channel-major
  // [row group][8 channels] image of rounds 1-4 put 8 lanes on one bank: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.77)
  __shared__ double sh[2][4][256];
  const int tx = threadIdx.x & 1, ty = threadIdx.x >> 1;
  double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
  const int c4 = cbase + tx * 4;
  if (c4 < Cp) {
#pragma unroll 4
    for (int k = ty; k < n; k += 128) {
      const float4 u = *reinterpret_cast<const float4*>(partial + ((size_t)k * 2 + 0) * Cp + c4);
      a0[0] += (double)u.x; a0[1] += (double)u.y; a0[2] += (double)u.z; a0[3] += (double)u.w;
      if (two) {
        const float4 v = *reinterpret_cast<const float4*>(partial + ((size_t)k * 2 + 1) * Cp + c4);
        a1[0] += (double)v.x; a1[1] += (double)v.y; a1[2] += (double)v.z; a1[3] += (double)v.w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { sh[0][j][threadIdx.x] = a0[j]; sh[1][j][threadIdx.x] = a1[j]; }
  __syncthreads();
  // waves 0 and 1 (which = 0, 1): lane l adds, per j, the entries of threads l, l + 64, l + 128, l + 192 (same tx = l & 1), then
  // a fixed shuffle tree over the 32 lanes of its parity: lanes 0 / 1 end with channels j / 4 + j
  __shared__ double res[2][8];
  if (threadIdx.x < 128) {
    const int l = threadIdx.x & 63, which = threadIdx.x >> 6;
    double a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = (sh[which][j][l] + sh[which][j][l + 64]) + (sh[which][j][l + 128] + sh[which][j][l + 192]);
      a[j] += __shfl_xor(a[j], 2);
      a[j] += __shfl_xor(a[j], 4);
      a[j] += __shfl_xor(a[j], 8);
      a[j] += __shfl_xor(a[j], 16);
      a[j] += __shfl_xor(a[j], 32);
    }
    if (l < 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) res[which][l * 4 + j] = a[j];
    }
  }
  __syncthreads();
  s0 = 0.0; s1 = 0.0;
  if (threadIdx.x < 8) { s0 = res[0][threadIdx.x]; s1 = res[1][threadIdx.x]; }
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partial, int ntiles, double count,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                   float momentum, float* running_mean, float* running_var, float* mean_o,
                                   float* rstd_o, float* scale_o, float* shift_o, float* bwd_coef, int C, int Cp,
                                   int training, long* batches_tracked) {
  // nn.BatchNorm1d.num_batches_tracked += 1 (models.py:135,143: track_running_stats) — here, not in a launch of its own
  if (batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *batches_tracked += 1;
  const int c = blockIdx.x * 8 + (threadIdx.x & 7);
  double s = 0.0, q = 0.0;
  if (training) block_partial_sums(partial, ntiles, Cp, blockIdx.x * 8, true, s, q);
  if (threadIdx.x >= 8 || c >= Cp) return;
  if (c >= C) {
    mean_o[c] = 0.f; rstd_o[c] = 0.f; scale_o[c] = 0.f; shift_o[c] = 0.f;
    if (bwd_coef) { bwd_coef[c] = 0.f; bwd_coef[Cp + c] = 0.f; bwd_coef[2 * Cp + c] = 0.f; bwd_coef[3 * Cp + c] = 0.f; }
    return;
  }
  double mean, var;
  if (training) {
    mean = s / count;
    var = q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    if (running_mean) {
      const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
      running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
      running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
    }
  } else {
    mean = running_mean[c];
    var = running_var[c];
  }
  const double rstd = 1.0 / sqrt(var + (double)eps);
  const double sc = (double)gamma[c] * rstd;
  mean_o[c] = (float)mean;
  rstd_o[c] = (float)rstd;
  scale_o[c] = (float)sc;
  shift_o[c] = (float)((double)beta[c] - mean * sc);
  if (bwd_coef) {
    bwd_coef[c] = gamma[c]; bwd_coef[Cp + c] = beta[c]; bwd_coef[2 * Cp + c] = (float)mean; bwd_coef[3 * Cp + c] = (float)rstd;
  }
}

template <typename E>
__global__ __launch_bounds__(256) void bn_gelu_fwd_kernel(const E* __restrict__ x, E* __restrict__ y,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int B, int T, int Cp) {
  constexpr int CH = Vec16<E>::N, U = 4;
  const int nch = Cp / CH;
  const int RG = nch >= 256 ? 1 : 256 / nch;
  int r0, r1;
  block_rows(B, T, r0, r1);
  for (int c = threadIdx.x; c < RG * nch; c += 256) {       // one pass unless a row has more than 256 chunks
    const int ch = c % nch, rg = c / nch;
    float sc[CH], sh[CH];
#pragma unroll
    for (int q4 = 0; q4 < CH / 4; ++q4) {
      *reinterpret_cast<float4*>(sc + q4 * 4) = *reinterpret_cast<const float4*>(scale + ch * CH + q4 * 4);
      *reinterpret_cast<float4*>(sh + q4 * 4) = *reinterpret_cast<const float4*>(shift + ch * CH + q4 * 4);
    }
    auto one = [&](float* v) {
#pragma unroll
      for (int j = 0; j < CH; j += 2) {
        const f32x2 o = gelu_pair<E>(fma2(f32x2{v[j], v[j + 1]}, f32x2{sc[j], sc[j + 1]}, f32x2{sh[j], sh[j + 1]}));
        v[j] = o.x; v[j + 1] = o.y;
      }
    };
    RowCursor w(r0, r1, rg, RG, T, Cp, ch * CH);
    for (; w.n >= U; w.n -= U) {
      uint32_t off[U];
      float v[U][CH];
#pragma unroll
      for (int u = 0; u < U; ++u) off[u] = w.take();
#pragma unroll
      for (int u = 0; u < U; ++u) Vec16<E>::load(x + off[u], v[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) { one(v[u]); Vec16<E>::store(y + off[u], v[u]); }
    }
    for (; w.n > 0; --w.n) {
      const uint32_t off = w.take();
      float v[CH];
      Vec16<E>::load(x + off, v);
      one(v);
      Vec16<E>::store(y + off, v);
    }
  }
}

constexpr int RED_MAX_BLOCKS = 1024;

// LDS image in which the per-row-group column sums of col_reduce_kernel and bwd_colsum_kernel meet: [row group][which][16-byte
// quarter q][chunk] float4, so a wave's store is 64 consecutive 16-byte slots (conflict-free; channel-major rows of CH floats
// per lane were 2- to 4-way conflicted).  A row group takes `rgs` float4: 2 * (CH / 4) * nch, plus bwd_colsum_pad for the kernel
// that asks for it.  The store, the sum over row groups and the byte count of the launch are the three below and nowhere else.

// padding (in float4) behind a row group: (2 * (CH / 4) * nch + pad) = nch (mod 16)
__host__ __device__ inline int bwd_colsum_pad(int nch, int CH) { return (((nch - 2 * (CH / 4) * nch) % 16) + 16) % 16; }
__host__ __device__ inline int colsum_rg_stride(int nch, int CH, bool padded) { return 2 * (CH / 4) * nch + (padded ? bwd_colsum_pad(nch, CH) : 0); }

template <int CH>
__device__ __forceinline__ void colsum_lds_store(float* red, int rgs, int rg, int nch, int ch, const float (&a0)[CH], const float (&a1)[CH]) {
#pragma unroll
  for (int q4 = 0; q4 < CH / 4; ++q4) {
    *reinterpret_cast<float4*>(red + ((rg * rgs + (0 * (CH / 4) + q4) * nch + ch) << 2)) = make_float4(a0[4 * q4], a0[4 * q4 + 1], a0[4 * q4 + 2], a0[4 * q4 + 3]);
    *reinterpret_cast<float4*>(red + ((rg * rgs + (1 * (CH / 4) + q4) * nch + ch) << 2)) = make_float4(a1[4 * q4], a1[4 * q4 + 1], a1[4 * q4 + 2], a1[4 * q4 + 3]);
  }
}
// partial[blockIdx.x][which][c] = sum over the RG row groups, in row-group order; `width` = CH * nch channels
template <int CH>
__device__ __forceinline__ void colsum_lds_sum(const float* red, int rgs, int RG, int nch, int width, float* __restrict__ partial) {
  for (int i = threadIdx.x; i < 2 * width; i += 256) {
    const int which = i / width, c = i - which * width;
    const int chc = c / CH, q4 = (c % CH) >> 2, e = c & 3;
    float sum = 0.f;
    for (int g = 0; g < RG; ++g) sum += red[((g * rgs + (which * (CH / 4) + q4) * nch + chc) << 2) + e];
    partial[((size_t)blockIdx.x * 2 + which) * width + c] = sum;
  }
}
// dynamic LDS of a launch over `width` channels of `dtype`: RG row groups as the kernels count them (RG = 256 / nch, so
// nch <= 256 — the entry points' width <= 1024 check is what keeps it so)
static inline size_t colsum_lds_bytes(int width, int dtype, bool padded) {
  const int CH = dtype == SDA_F32 ? 4 : 8, nch = width / CH, RG = 256 / nch;
  return (size_t)RG * colsum_rg_stride(nch, CH, padded) * 16;
}

// Column reductions over valid rows.  MODE 0: sum x (bias grads).  MODE 1: BN+GELU backward sums
// (dg, dg * xhat) with dg = dy * GELU'(gamma * xhat + beta).
template <typename E, int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(const E* __restrict__ dy, const E* __restrict__ x,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int C, float* __restrict__ partial, int B, int T, int Cp) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  constexpr int CH = Vec16<E>::N;
  const int nch = Cp / CH;
  const int RG = 256 / nch;
  const int ch = threadIdx.x % nch, rg = threadIdx.x / nch;
  const size_t rows = (size_t)B * T;
  const size_t per = (rows + gridDim.x - 1) / gridDim.x;
  const size_t r0 = (size_t)blockIdx.x * per, r1 = min(rows, r0 + per);
  float a0[CH], a1[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) { a0[j] = 0.f; a1[j] = 0.f; }
  if (rg < RG) {
    float mu[CH], rs[CH], ga[CH], be[CH];
    if (MODE == 1) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int c = ch * CH + j;
        mu[j] = mean[c]; rs[j] = rstd[c];
        ga[j] = c < C ? gamma[c] : 0.f; be[j] = c < C ? beta[c] : 0.f;
      }
    }
#pragma unroll 2
    for (RowWalk w((int)r0 + rg, (int)r1, RG, T); w.valid(); w.next()) {
      const size_t off = w.mem_row() * Cp + ch * CH;
      float dv[CH];
      Vec16<E>::load(dy + off, dv);
      if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < CH; ++j) a0[j] += dv[j];
      } else {
        float xv[CH];
        Vec16<E>::load(x + off, xv);
#pragma unroll
        for (int j = 0; j < CH; j += 2) {
          const f32x2 xh = (f32x2{xv[j], xv[j + 1]} - f32x2{mu[j], mu[j + 1]}) * f32x2{rs[j], rs[j + 1]};
          const f32x2 dg = f32x2{dv[j], dv[j + 1]} * gelu_grad_pair<E>(fma2(f32x2{ga[j], ga[j + 1]}, xh, f32x2{be[j], be[j + 1]}));
          const f32x2 dgx = dg * xh;
          a0[j] += dg.x; a0[j + 1] += dg.y;
          a1[j] += dgx.x; a1[j + 1] += dgx.y;
        }
      }
    }
  }
  const int rgs = colsum_rg_stride(nch, CH, false);
  if (rg < RG) colsum_lds_store<CH>(red, rgs, rg, nch, ch, a0, a1);
  __syncthreads();
  colsum_lds_sum<CH>(red, rgs, RG, nch, Cp, partial);
}

// Backward elementwise stage fused with the column sums of its own output (bias gradients of the layer
// below), same thread->channel ownership as col_reduce_kernel.
//   MODE 0 (GELU):  du = dz * GELU'(u);  partial[blk][0][c] = sum du
//   MODE 1 (GLU):   x = [a | g] (2*Ch channels), dy (Ch): da = dy*sig(g), dg = dy*a*sig(g)*(1-sig(g));
//                   partial[blk][0][c] = sum da, partial[blk][1][c] = sum dg      (c < Ch)
//   MODE 2 (GLU after a fused forward, SDA_EPI_GLU): x = out = a*sig(g) (Ch channels), gate = g (Ch channels):
//                   da = dy*sig(g), dg = dy*out*(1-sig(g)); same outputs as MODE 1 (the value half is never stored)
template <typename E, int MODE>
__global__ __launch_bounds__(256) void bwd_colsum_kernel(const E* __restrict__ x, const E* __restrict__ dy,
                                                         E* __restrict__ dx, float* __restrict__ partial, int B, int T,
                                                         int Ch, const E* __restrict__ gate = nullptr) {
  ew_bwd_prio();
  extern __shared__ __attribute__((aligned(16))) float red[];
  constexpr int CH = Vec16<E>::N;
  const int nch = Ch / CH;
  const int RG = 256 / nch;
  const int ch = threadIdx.x % nch, rg = threadIdx.x / nch;
  const size_t rows = (size_t)B * T;
  const size_t per = (rows + gridDim.x - 1) / gridDim.x;
  const size_t r0 = (size_t)blockIdx.x * per, r1 = min(rows, r0 + per);
  const int xw = MODE == 1 ? 2 * Ch : Ch, dxw = MODE == 0 ? Ch : 2 * Ch;
  float a0[CH], a1[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) { a0[j] = 0.f; a1[j] = 0.f; }
  if (rg < RG) {
    RowCursor w((int)r0, (int)r1, rg, RG, T, Ch, ch * CH);       // offsets in Ch-wide rows; 2*Ch-wide rows: 2 * off - ch * CH
#pragma unroll 2
    for (; w.n > 0; --w.n) {
      const uint32_t off = w.take(), off2 = 2 * off - ch * CH;
      float d[CH], xv[CH], o0[CH], o1[CH];
      Vec16<E>::load(dy + off, d);
      Vec16<E>::load(x + (MODE == 1 ? off2 : off), xv);
      if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < CH; j += 2) {
          const f32x2 o = f32x2{d[j], d[j + 1]} * gelu_grad_pair<E>(f32x2{xv[j], xv[j + 1]});
          o0[j] = o.x; o0[j + 1] = o.y;
          a0[j] += o.x; a0[j + 1] += o.y;
        }
        Vec16<E>::store(dx + off, o0);
      } else {
        float g[CH];
        if (MODE == 1) Vec16<E>::load(x + off2 + Ch, g);
        else Vec16<E>::load(gate + off, g);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const float sg = sigmoid_f(g[j]);
          o0[j] = d[j] * sg;
          o1[j] = MODE == 1 ? d[j] * xv[j] * sg * (1.f - sg) : d[j] * xv[j] * (1.f - sg);
          a0[j] += o0[j];
          a1[j] += o1[j];
        }
        Vec16<E>::store(dx + off2, o0);
        Vec16<E>::store(dx + off2 + Ch, o1);
      }
    }
  }
  // (the padded image: a row group's base is shifted so that base(rg + 1) = base(rg) + nch (mod 16 float4): the 16 lanes of a
  // store that straddle two row groups — 320 channels: nch = 40, lanes 32..47 = chunks 32..39 of one group and 0..7 of the
  // next — then still take 16 distinct 16-byte slots of a bank row)
  const int rgs = colsum_rg_stride(nch, CH, true);
  if (rg < RG) colsum_lds_store<CH>(red, rgs, rg, nch, ch, a0, a1);
  __syncthreads();
  colsum_lds_sum<CH>(red, rgs, RG, nch, Ch, partial);
}

// sums[which][c] = sum over blocks (fp64, fixed order)
__global__ __launch_bounds__(256) void col_reduce_final_kernel(const float* __restrict__ partial, int nblocks,
                                                               float* __restrict__ out0, float* __restrict__ out1, int Cp) {
  ew_bwd_prio();
  const int c = blockIdx.x * 8 + (threadIdx.x & 7);
  double s0, s1;
  block_partial_sums(partial, nblocks, Cp, blockIdx.x * 8, out1 != nullptr, s0, s1);
  if (threadIdx.x >= 8 || c >= Cp) return;
  out0[c] = (float)s0;
  if (out1) out1[c] = (float)s1;
}

// per-channel coefficients of the BN+GELU backward, precomputed once per launch into a [6][Cp] table:
//   0: gamma  1: beta  2: mean  3: rstd  4: dbeta/N  5: dgamma/N
// (written by both kernels below: through a shared writer bn_bwd_coef_kernel loads dbeta and dgamma ahead of its stores, and
// the reduce_stats + coefficients + apply chain over a bf16 (256, 320, 360) buffer takes 37.4 us instead of 36.9)
__global__ void bn_bwd_coef_kernel(const float* __restrict__ mean, const float* __restrict__ rstd,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, int C,
                                   const float* __restrict__ dbeta, const float* __restrict__ dgamma, float inv_count,
                                   float* __restrict__ coef, int Cp) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Cp) return;
  coef[0 * Cp + c] = c < C ? gamma[c] : 0.f;
  coef[1 * Cp + c] = c < C ? beta[c] : 0.f;
  coef[2 * Cp + c] = mean[c];
  coef[3 * Cp + c] = rstd[c];
  // eval mode hands in 1 / N = 0 (no batch-statistics terms): a select, since 0 * the sums would carry one sample's inf / NaN into all
  coef[4 * Cp + c] = inv_count != 0.f ? dbeta[c] * inv_count : 0.f;
  coef[5 * Cp + c] = inv_count != 0.f ? dgamma[c] * inv_count : 0.f;
}

// reduce_stats + bn_bwd_coef in one launch (single-process case: no all-reduce sits between them)
__global__ __launch_bounds__(256) void bn_bwd_stats_coef_kernel(const float* __restrict__ partial, int nrows,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                int C, float inv_count, float* __restrict__ dbeta,
                                                                float* __restrict__ dgamma, float* __restrict__ coef, int Cp) {
  ew_bwd_prio();
  const int c = blockIdx.x * 8 + (threadIdx.x & 7);
  double s0, s1;
  block_partial_sums(partial, nrows, Cp, blockIdx.x * 8, true, s0, s1);
  if (threadIdx.x >= 8 || c >= Cp) return;
  const float db = (float)s0, dg = (float)s1;
  dbeta[c] = db;
  dgamma[c] = dg;
  coef[0 * Cp + c] = c < C ? gamma[c] : 0.f;
  coef[1 * Cp + c] = c < C ? beta[c] : 0.f;
  coef[2 * Cp + c] = mean[c];
  coef[3 * Cp + c] = rstd[c];
  coef[4 * Cp + c] = inv_count != 0.f ? db * inv_count : 0.f;          // (a select: see bn_bwd_coef_kernel)
  coef[5 * Cp + c] = inv_count != 0.f ? dg * inv_count : 0.f;
}

// DG: `dy` already holds dg = dy * GELU'(gamma * xhat + beta) (a conv epilogue with SDA_EPI_BN_STORE_DG wrote it): the affine
// part only — 5 vector instructions per element pair instead of ~25
template <typename E, bool DG = false>
__global__ __launch_bounds__(256) void bn_gelu_bwd_apply_kernel(const E* __restrict__ dy, const E* __restrict__ x,
                                                                const float* __restrict__ coef, E* __restrict__ dx,
                                                                int B, int T, int Cp) {
  ew_bwd_prio();
  constexpr int CH = Vec16<E>::N, U = 2;
  const int nch = Cp / CH;
  const int RG = nch >= 256 ? 1 : 256 / nch;
  int r0, r1;
  block_rows(B, T, r0, r1);
  for (int c = threadIdx.x; c < RG * nch; c += 256) {
    const int ch = c % nch, rg = c / nch;
    // per channel: a = gamma*rstd, b = beta - a*mean (so gamma*xhat + beta = a*x + b), and the linear part of
    //   dx = gamma*rstd*(g - dbeta/N - xhat*dgamma/N) = a*g - (p + q*x),  q = a*rstd*dgamma/N,  p = a*dbeta/N - q*mean
    float ca[CH], cb[CH], cp[CH], cq[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int k = ch * CH + j;
      const float ga = coef[k], be = coef[Cp + k], mu = coef[2 * Cp + k], rs = coef[3 * Cp + k];
      ca[j] = ga * rs;
      cb[j] = be - ca[j] * mu;
      cq[j] = ca[j] * rs * coef[5 * Cp + k];
      cp[j] = ca[j] * coef[4 * Cp + k] - cq[j] * mu;
    }
    auto one = [&](float* d, const float* xv) {
#pragma unroll
      for (int j = 0; j < CH; j += 2) {
        const f32x2 xx = {xv[j], xv[j + 1]}, a2 = {ca[j], ca[j + 1]};
        f32x2 g = f32x2{d[j], d[j + 1]};
        if constexpr (!DG) g = g * gelu_grad_pair<E>(fma2(a2, xx, f32x2{cb[j], cb[j + 1]}));
        const f32x2 o = fma2(a2, g, -fma2(f32x2{cq[j], cq[j + 1]}, xx, f32x2{cp[j], cp[j + 1]}));
        d[j] = o.x; d[j + 1] = o.y;
      }
    };
    RowCursor w(r0, r1, rg, RG, T, Cp, ch * CH);
    for (; w.n >= U; w.n -= U) {
      uint32_t off[U];
      float d[U][CH], xv[U][CH];
#pragma unroll
      for (int u = 0; u < U; ++u) off[u] = w.take();
#pragma unroll
      for (int u = 0; u < U; ++u) { Vec16<E>::load(dy + off[u], d[u]); Vec16<E>::load(x + off[u], xv[u]); }
#pragma unroll
      for (int u = 0; u < U; ++u) { one(d[u], xv[u]); Vec16<E>::store(dx + off[u], d[u]); }
    }
    for (; w.n > 0; --w.n) {
      const uint32_t off = w.take();
      float d[CH], xv[CH];
      Vec16<E>::load(dy + off, d);
      Vec16<E>::load(x + off, xv);
      one(d, xv);
      Vec16<E>::store(dx + off, d);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// GLU (models.py:164) and GELU backward
// ------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void glu_fwd_kernel(const E* __restrict__ x, E* __restrict__ y, int B, int T, int Ch) {
  constexpr int CH = Vec16<E>::N, U = 2;
  const int nch = Ch / CH;
  const int RG = nch >= 256 ? 1 : 256 / nch;
  int r0, r1;
  block_rows(B, T, r0, r1);
  for (int c = threadIdx.x; c < RG * nch; c += 256) {
    const int ch = c % nch, rg = c / nch;
    RowCursor w(r0, r1, rg, RG, T, Ch, ch * CH);            // offsets in the Ch-wide output; the input row is twice as wide
    auto one = [&](uint32_t off) {
      float a[CH], g[CH];
      const uint32_t xo = 2 * off - ch * CH;                // row * 2 Ch + ch * CH
      Vec16<E>::load(x + xo, a);
      Vec16<E>::load(x + xo + Ch, g);
#pragma unroll
      for (int j = 0; j < CH; ++j) a[j] *= sigmoid_f(g[j]);
      Vec16<E>::store(y + off, a);
    };
    for (; w.n >= U; w.n -= U) {
      uint32_t off[U];
#pragma unroll
      for (int u = 0; u < U; ++u) off[u] = w.take();
#pragma unroll
      for (int u = 0; u < U; ++u) one(off[u]);
    }
    for (; w.n > 0; --w.n) one(w.take());
  }
}

template <typename E>
__global__ __launch_bounds__(256) void glu_bwd_kernel(const E* __restrict__ x, const E* __restrict__ dy,
                                                      E* __restrict__ dx, int B, int T, int Ch) {
  constexpr int CH = Vec16<E>::N;
  const int nch = Ch / CH;
  const int RG = nch >= 256 ? 1 : 256 / nch;
  int r0, r1;
  block_rows(B, T, r0, r1);
  for (int c = threadIdx.x; c < RG * nch; c += 256) {
    const int ch = c % nch, rg = c / nch;
    for (RowWalk w(r0 + rg, r1, RG, T); w.valid(); w.next()) {
      const size_t row = w.mem_row();
      float a[CH], g[CH], d[CH];
      Vec16<E>::load(x + row * 2 * Ch + ch * CH, a);
      Vec16<E>::load(x + row * 2 * Ch + Ch + ch * CH, g);
      Vec16<E>::load(dy + row * Ch + ch * CH, d);
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float sg = sigmoid_f(g[j]);
        g[j] = d[j] * a[j] * sg * (1.f - sg);               // same expression order as bwd_colsum_kernel<1> (bit-equal outputs)
        a[j] = d[j] * sg;
      }
      Vec16<E>::store(dx + row * 2 * Ch + ch * CH, a);
      Vec16<E>::store(dx + row * 2 * Ch + Ch + ch * CH, g);
    }
  }
}

template <typename E>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const E* __restrict__ u, const E* __restrict__ dz,
                                                       E* __restrict__ du, int B, int T, int Cp) {
  constexpr int CH = Vec16<E>::N;
  const int nch = Cp / CH;
  const int RG = nch >= 256 ? 1 : 256 / nch;
  int r0, r1;
  block_rows(B, T, r0, r1);
  for (int c = threadIdx.x; c < RG * nch; c += 256) {
    const int ch = c % nch, rg = c / nch;
    for (RowWalk w(r0 + rg, r1, RG, T); w.valid(); w.next()) {
      const size_t off = w.mem_row() * Cp + ch * CH;
      float uv[CH], d[CH];
      Vec16<E>::load(u + off, uv);
      Vec16<E>::load(dz + off, d);
#pragma unroll
      for (int j = 0; j < CH; j += 2) {
        const f32x2 o = f32x2{d[j], d[j + 1]} * gelu_grad_pair<E>(f32x2{uv[j], uv[j + 1]});
        d[j] = o.x; d[j + 1] = o.y;
      }
      Vec16<E>::store(du + off, d);
    }
  }
}

static int red_blocks(int B, int T) {
  long rows = (long)B * T;
  long nb = (rows + 31) / 32;
  if (nb > RED_MAX_BLOCKS) nb = RED_MAX_BLOCKS;
  if (nb < 1) nb = 1;
  return (int)nb;
}

}  // namespace sda

using namespace sda;

extern "C" int sda_rows_sumsq_from_stats(const float* stats, int tiles_per_sample, int Cp, float* out, int B, void* stream) {
  if (!stats || !out || tiles_per_sample < 1 || Cp < 1 || B < 1) { set_error("rows_sumsq_from_stats: bad arguments"); return -1; }
  hipLaunchKernelGGL(rows_sumsq_from_stats_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, stats, tiles_per_sample, Cp, out);
  return check_launch("rows_sumsq_from_stats");
}

extern "C" int sda_rows_sumsq_from_row_parts(const float* parts, int n_parts, float* out, int B, int T, void* stream) {
  if (!parts || !out || n_parts < 1 || B < 1 || T < 1) { set_error("rows_sumsq_from_row_parts: bad arguments"); return -1; }
  hipLaunchKernelGGL(rows_sumsq_from_row_parts_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, parts, n_parts, T, out);
  return check_launch("rows_sumsq_from_row_parts");
}

extern "C" int sda_rows_sumsq(const void* x, float* out, float* scratch, int B, long row_elems, long pitch,
                              int dtype, void* stream) {
  if (!x || !out || !scratch || row_elems % 4 || pitch % 4 || B < 1) { set_error("rows_sumsq: bad arguments"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(rows_sumsq_kernel<E>, dim3(SUMSQ_CHUNKS, B), dim3(256), 0, st,
                                         (const E*)x, scratch, row_elems, pitch));
  hipLaunchKernelGGL(rows_sumsq_final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, out, B);
  return check_launch("rows_sumsq");
}

extern "C" int sda_bn_finalize(const float* partial, int ntiles, double count, const float* gamma, const float* beta,
                               float eps, float momentum, float* running_mean, float* running_var, float* mean,
                               float* rstd, float* scale, float* shift, float* bwd_coef, int C, int Cp, int training,
                               long* batches_tracked, void* stream) {
  if (!gamma || !beta || !mean || !rstd || !scale || !shift || C > Cp) { set_error("bn_finalize: bad arguments"); return -1; }
  if (training && (!partial || ntiles < 1 || count < 1.0)) { set_error("bn_finalize: training mode needs partial statistics"); return -1; }
  if (!training && (!running_mean || !running_var)) { set_error("bn_finalize: eval mode needs running statistics"); return -1; }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((Cp + 7) / 8), dim3(256), 0, (hipStream_t)stream, partial, ntiles, count,
                     gamma, beta, eps, momentum, running_mean, running_var, mean, rstd, scale, shift, bwd_coef, C, Cp,
                     training, training ? batches_tracked : nullptr);
  return check_launch("bn_finalize");
}

extern "C" int sda_bn_gelu_forward(const void* x, void* y, const float* scale, const float* shift, int B, int T,
                                   int Cp, int dtype, void* stream) {
  if (!x || !y || !scale || !shift || Cp % 64 || !fits_u32(B, T, Cp)) { set_error("bn_gelu_forward: bad arguments"); return -1; }
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(bn_gelu_fwd_kernel<E>, dim3(stream_blocks(B, T, Cp / Vec16<E>::N)), dim3(256), 0, (hipStream_t)stream,
                                         (const E*)x, (E*)y, scale, shift, B, T, Cp));
  return check_launch("bn_gelu_forward");
}

// col_reduce_kernel<E, MODE> into `partial`, then the sum over its blocks into out0 (and out1, unless null)
template <int MODE>
static int launch_col_reduce(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                             const float* beta, int C, float* partial, float* out0, float* out1, int B, int T, int Cp,
                             int dtype, hipStream_t st) {
  const int nb = red_blocks(B, T);
  SDA_DISPATCH(dtype, hipLaunchKernelGGL((col_reduce_kernel<E, MODE>), dim3(nb), dim3(256), colsum_lds_bytes(Cp, dtype, false), st,
                                         (const E*)dy, (const E*)x, mean, rstd, gamma, beta, C, partial, B, T, Cp));
  hipLaunchKernelGGL(col_reduce_final_kernel, dim3((Cp + 7) / 8), dim3(256), 0, st, partial, nb, out0, out1, Cp);
  return 0;
}

extern "C" int sda_bn_gelu_backward_reduce(const void* dy, const void* x, const float* mean, const float* rstd,
                                           const float* gamma, const float* beta, int C, float* partial, float* dgamma,
                                           float* dbeta, int B, int T, int Cp, int dtype, void* stream) {
  if (!dy || !x || !mean || !rstd || !gamma || !beta || !partial || !dgamma || !dbeta || Cp % 64 || Cp > 1024) {
    set_error("bn_gelu_backward_reduce: bad arguments"); return -1;
  }
  if (launch_col_reduce<1>(dy, x, mean, rstd, gamma, beta, C, partial, dbeta, dgamma, B, T, Cp, dtype, (hipStream_t)stream)) return -1;
  return check_launch("bn_gelu_backward_reduce");
}

extern "C" int sda_reduce_stats(const float* partial, int nrows, float* out0, float* out1, int Cp, void* stream) {
  if (!partial || !out0 || nrows < 1 || Cp % 8) { set_error("reduce_stats: bad arguments"); return -1; }
  hipLaunchKernelGGL(col_reduce_final_kernel, dim3((Cp + 7) / 8), dim3(256), 0, (hipStream_t)stream, partial, nrows,
                     out0, out1, Cp);
  return check_launch("reduce_stats");
}

// bn_gelu_bwd_apply_kernel<E, dg> over the coefficient table a launch in front of it wrote
static int launch_bn_bwd_apply(bool dg, const void* dy, const void* x, const float* coef, void* dx, int B, int T, int Cp,
                               int dtype, hipStream_t st) {
  SDA_DISPATCH(dtype, hipLaunchKernelGGL((dg ? bn_gelu_bwd_apply_kernel<E, true> : bn_gelu_bwd_apply_kernel<E, false>),
                                         dim3(stream_blocks(B, T, Cp / Vec16<E>::N)), dim3(256), 0, st, (const E*)dy, (const E*)x, coef,
                                         (E*)dx, B, T, Cp));
  return 0;
}

static int bn_backward_apply(bool dg, const void* dy, const void* x, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, int C, const float* dgamma,
                             const float* dbeta, double count, float* coef, void* dx, int B, int T, int Cp,
                             int dtype, void* stream) {
  if (!dy || !x || !mean || !rstd || !gamma || !beta || !dgamma || !dbeta || !coef || !dx || Cp % 64 || count < 1.0 || !fits_u32(B, T, Cp)) {
    set_error("bn_gelu_backward_apply: bad arguments"); return -1;
  }
  const float inv_count = (float)(1.0 / count);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((Cp + 255) / 256), dim3(256), 0, st, mean, rstd, gamma, beta, C, dbeta,
                     dgamma, inv_count, coef, Cp);
  if (launch_bn_bwd_apply(dg, dy, x, coef, dx, B, T, Cp, dtype, st)) return -1;
  return check_launch("bn_gelu_backward_apply");
}

extern "C" int sda_bn_gelu_backward_apply(const void* dy, const void* x, const float* mean, const float* rstd,
                                          const float* gamma, const float* beta, int C, const float* dgamma,
                                          const float* dbeta, double count, float* coef, void* dx, int B, int T, int Cp,
                                          int dtype, void* stream) {
  return bn_backward_apply(false, dy, x, mean, rstd, gamma, beta, C, dgamma, dbeta, count, coef, dx, B, T, Cp, dtype, stream);
}
extern "C" int sda_bn_gelu_backward_apply_dg(const void* dg, const void* x, const float* mean, const float* rstd,
                                             const float* gamma, const float* beta, int C, const float* dgamma,
                                             const float* dbeta, double count, float* coef, void* dx, int B, int T, int Cp,
                                             int dtype, void* stream) {
  return bn_backward_apply(true, dg, x, mean, rstd, gamma, beta, C, dgamma, dbeta, count, coef, dx, B, T, Cp, dtype, stream);
}

static int bn_backward_from_stats(bool dg, const float* partial, int nrows, const void* dy, const void* x,
                                  const float* mean, const float* rstd, const float* gamma,
                                  const float* beta, int C, double count, float* dgamma, float* dbeta,
                                  float* coef, void* dx, int B, int T, int Cp, int dtype, void* stream) {
  if (!partial || nrows < 1 || !dy || !x || !mean || !rstd || !gamma || !beta || !dgamma || !dbeta || !coef || !dx ||
      Cp % 64 || count < 1.0 || !fits_u32(B, T, Cp)) {
    set_error("bn_gelu_backward_from_stats: bad arguments"); return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_bwd_stats_coef_kernel, dim3((Cp + 7) / 8), dim3(256), 0, st, partial, nrows, mean, rstd, gamma, beta, C,
                     (float)(1.0 / count), dbeta, dgamma, coef, Cp);
  if (launch_bn_bwd_apply(dg, dy, x, coef, dx, B, T, Cp, dtype, st)) return -1;
  return check_launch("bn_gelu_backward_from_stats");
}

extern "C" int sda_bn_gelu_backward_from_stats(const float* partial, int nrows, const void* dy, const void* x,
                                              const float* mean, const float* rstd, const float* gamma,
                                              const float* beta, int C, double count, float* dgamma, float* dbeta,
                                              float* coef, void* dx, int B, int T, int Cp, int dtype, void* stream) {
  return bn_backward_from_stats(false, partial, nrows, dy, x, mean, rstd, gamma, beta, C, count, dgamma, dbeta, coef, dx, B, T, Cp, dtype, stream);
}
extern "C" int sda_bn_gelu_backward_from_stats_dg(const float* partial, int nrows, const void* dg, const void* x,
                                                 const float* mean, const float* rstd, const float* gamma,
                                                 const float* beta, int C, double count, float* dgamma, float* dbeta,
                                                 float* coef, void* dx, int B, int T, int Cp, int dtype, void* stream) {
  return bn_backward_from_stats(true, partial, nrows, dg, x, mean, rstd, gamma, beta, C, count, dgamma, dbeta, coef, dx, B, T, Cp, dtype, stream);
}

extern "C" int sda_colsum(const void* x, float* out, float* scratch, int B, int T, int Cp, int dtype, void* stream) {
  if (!x || !out || !scratch || Cp % 64 || Cp > 1024) { set_error("colsum: bad arguments"); return -1; }
  if (launch_col_reduce<0>(x, nullptr, nullptr, nullptr, nullptr, nullptr, 0, scratch, out, nullptr, B, T, Cp, dtype, (hipStream_t)stream)) return -1;
  return check_launch("colsum");
}

extern "C" int sda_reduce_scratch_floats(int Cp) { return RED_MAX_BLOCKS * 2 * Cp; }
extern "C" int sda_reduce_scratch_rows(int B, int T) { return red_blocks(B, T); }

extern "C" int sda_glu_forward(const void* x, void* y, int B, int T, int Ch, int dtype, void* stream) {
  if (!x || !y || Ch % 64 || !fits_u32(B, T, 2L * Ch)) { set_error("glu_forward: bad arguments"); return -1; }
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(glu_fwd_kernel<E>, dim3(stream_blocks(B, T, Ch / Vec16<E>::N)), dim3(256), 0, (hipStream_t)stream,
                                         (const E*)x, (E*)y, B, T, Ch));
  return check_launch("glu_forward");
}

extern "C" int sda_glu_backward(const void* x, const void* dy, void* dx, int B, int T, int Ch, int dtype, void* stream) {
  if (!x || !dy || !dx || Ch % 64) { set_error("glu_backward: bad arguments"); return -1; }
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(glu_bwd_kernel<E>, dim3(stream_blocks(B, T, Ch / Vec16<E>::N)), dim3(256), 0, (hipStream_t)stream,
                                         (const E*)x, (const E*)dy, (E*)dx, B, T, Ch));
  return check_launch("glu_backward");
}

extern "C" int sda_gelu_backward(const void* u, const void* dz, void* du, int B, int T, int Cp, int dtype, void* stream) {
  if (!u || !dz || !du || Cp % 64) { set_error("gelu_backward: bad arguments"); return -1; }
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(gelu_bwd_kernel<E>, dim3(stream_blocks(B, T, Cp / Vec16<E>::N)), dim3(256), 0, (hipStream_t)stream,
                                         (const E*)u, (const E*)dz, (E*)du, B, T, Cp));
  return check_launch("gelu_backward");
}

// bwd_colsum_kernel<E, MODE> with its per-block sums into `scratch`; with `colsum`, the sum over the blocks behind it
// (MODE 0: Ch sums; MODE 1 and 2: the value half's Ch, then the gate half's)
template <int MODE>
static int launch_bwd_colsum(const void* x, const void* dy, void* dx, const void* gate, float* colsum, float* scratch, int B, int T,
                             int Ch, int dtype, hipStream_t st) {
  const int nb = red_blocks(B, T);
  SDA_DISPATCH(dtype, hipLaunchKernelGGL((bwd_colsum_kernel<E, MODE>), dim3(nb), dim3(256), colsum_lds_bytes(Ch, dtype, true), st,
                                         (const E*)x, (const E*)dy, (E*)dx, scratch, B, T, Ch, (const E*)gate));
  if (colsum) hipLaunchKernelGGL(col_reduce_final_kernel, dim3((Ch + 7) / 8), dim3(256), 0, st, scratch, nb, colsum,
                                 MODE == 0 ? (float*)nullptr : colsum + Ch, Ch);
  return 0;
}

extern "C" int sda_glu_backward_colsum(const void* x, const void* dy, void* dx, float* colsum, float* scratch, int B, int T,
                                       int Ch, int dtype, void* stream) {
  if (!x || !dy || !dx || !scratch || Ch % 64 || Ch > 1024 || !fits_u32(B, T, 2L * Ch)) { set_error("glu_backward_colsum: bad arguments"); return -1; }
  if (launch_bwd_colsum<1>(x, dy, dx, nullptr, colsum, scratch, B, T, Ch, dtype, (hipStream_t)stream)) return -1;
  return check_launch("glu_backward_colsum");
}

extern "C" int sda_glu_backward_colsum_og(const void* out, const void* gate, const void* dy, void* dx, float* colsum,
                                          float* scratch, int B, int T, int Ch, int dtype, void* stream) {
  if (!out || !gate || !dy || !dx || !scratch || Ch % 64 || Ch > 1024 || !fits_u32(B, T, 2L * Ch)) { set_error("glu_backward_colsum_og: bad arguments"); return -1; }
  if (launch_bwd_colsum<2>(out, dy, dx, gate, colsum, scratch, B, T, Ch, dtype, (hipStream_t)stream)) return -1;
  return check_launch("glu_backward_colsum_og");
}

extern "C" int sda_gelu_backward_colsum(const void* u, const void* dz, void* du, float* colsum, float* scratch, int B, int T,
                                        int Cp, int dtype, void* stream) {
  if (!u || !dz || !du || !scratch || Cp % 64 || Cp > 1024 || !fits_u32(B, T, Cp)) { set_error("gelu_backward_colsum: bad arguments"); return -1; }
  if (launch_bwd_colsum<0>(u, dz, du, nullptr, colsum, scratch, B, T, Cp, dtype, (hipStream_t)stream)) return -1;
  return check_launch("gelu_backward_colsum");
}

