// window_gemm — a fixed matrix applied to strided, overlapping windows of each input row (fp32, exact-fp32 MFMA):
//
//     out[r][m * N + j] = sum_{k < K} x[r][m * S + k] * B[k][j]          r < rows, m < frames, j < N
//
// What it replaces: the two signal-conditioning convolutions in front of the training data — the zero-phase FIR band-pass
// of the raw recordings (mne.filter.filter_data, gwilliams2022.py:253 / brennan2018.py:263) and the polyphase sinc resampler
// of the audio (torchaudio.functional.resample, gwilliams2022.py:349 / brennan2018.py:172).  Both are this formula: the
// resampler with S = reduced input rate, N = reduced output rate, B = bank^T; the FIR as the degenerate resampler
// S = N = 1 with G consecutive frames grouped into one (S' = N' = G, B' the (K + G - 1) x G Toeplitz matrix of the taps),
// which is what makes it matrix-shaped (signal_prep.window_matrix builds B' and picks G).
//
// One workgroup = 4 waves owns 128 consecutive frames of one row x 64 output columns; wave w owns frames [32 w, 32 w + 32) on
// the M index of v_mfma_f32_32x32x2_f32 (lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]) and keeps
// two independent 32 x 32 accumulators (columns [0, 32) and [32, 64) of the tile), so one A fragment feeds two MFMAs.
//
// x.  The windows of a workgroup's frames overlap (K > S): their union, the SPAN x[m0 * S + k0 ... + 127 * S + KX), is staged
// in LDS once per KX-wide slice of the contraction and the MFMA's k slides along it: lane i reads xs[i * S + k].  When S is a
// multiple of 32 words every lane of that read would hit one bank (the grouped FIR's S = G = 64 is that case), so the image
// is skewed by one pad word per 64: position p lives at p + (p >> 6).  KX is the largest multiple of 32 the LDS budget leaves
// (the whole K for the FIR: 127 * 64 + 3364 floats).  When even the smallest slice does not fit (127 * S alone exceeds the
// budget: S > ~90, the audio's S = 441) the frames' windows are staged side by side instead, 64 k at a time with an odd
// pitch of 65 — no reuse to lose there, K / S is small.  Both forms are one compute loop: lane i reads xs[skew(i * SL + k)].
// B.  Constant and L2-resident (under 1 MB); streamed in 32-row chunks: global -> registers while the previous chunk
// computes -> LDS [32][64], rows k >= K and columns j >= N zero-filled.  A's k tail is masked in registers (a staged
// position past a frame's window belongs to the next frame's window: it holds data, not zero).
// Nothing is read outside x[r][0 ... (frames - 1) * S + K - 1] and nothing written outside out[r][0 ... frames * N - 1];
// ragged frame / column edges are masked at the store.  Results are a k-ordered fmaf chain per output: bitwise reproducible.
#include "sd_common.h"

namespace sda {

namespace {

constexpr int WG_TM = 128;               // frames per workgroup (32 per wave)
constexpr int WG_TN = 64;                // output columns per workgroup (two 32-wide accumulators per wave)
constexpr int WG_BK = 32;                // rows of B per chunk
constexpr int WG_XS = 12544;             // floats of the x image: 49 KiB; with B's 8 KiB two workgroups share a CU
constexpr int WG_SIDE_KX = 64;           // side-by-side form: k per slice ...
constexpr int WG_SIDE_PITCH = 65;        // ... and the (odd) pitch of a frame's piece

struct WgArgs {
  const float* x;
  const float* B;
  float* out;
  long x_row_stride, out_row_stride, frames;
  int rows, S, K, N;
  int tiles_n;
  long tiles_m;
  int KX;            // k per staged slice of x (a multiple of WG_BK)
  int SL;            // image stride between consecutive frames: S (span form) or WG_SIDE_PITCH
  int span;          // 1: span form, skewed image
};

__device__ __forceinline__ int wg_skew(int p, int sh) { return p + (p >> sh); }

__global__ __launch_bounds__(256) void window_gemm_kernel(const WgArgs a) {
  __shared__ float xs[WG_XS];
  __shared__ float Bs[WG_BK * WG_TN];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  long bid = blockIdx.x;
  const int nt = (int)(bid % a.tiles_n);
  bid /= a.tiles_n;
  const long mt = bid % a.tiles_m;
  const int r = (int)(bid / a.tiles_m);
  const long m0 = mt * WG_TM;
  const int j0 = nt * WG_TN;
  const float* __restrict__ xr = a.x + (size_t)r * a.x_row_stride;
  const long x_last = (a.frames - 1) * (long)a.S + a.K - 1;            // last readable element of a row
  const int sh = a.span ? 6 : 31;

  // B chunk: element e of this thread = row (tid >> 6) + 4 e of the chunk, column tid & 63 (coalesced along j)
  const int bj = j0 + lane;
  float rb[WG_BK / 4];
  auto fetch_b = [&](int k0) {
#pragma unroll
    for (int e = 0; e < WG_BK / 4; ++e) {
      const int k = k0 + wid + 4 * e;
      rb[e] = (k < a.K && bj < a.N) ? a.B[(size_t)k * a.N + bj] : 0.f;
    }
  };
  auto stash_b = [&]() {
#pragma unroll
    for (int e = 0; e < WG_BK / 4; ++e) Bs[(wid + 4 * e) * WG_TN + lane] = rb[e];
  };
  // x image of the slice [k0, k0 + kxn) of the contraction
  auto stage_x = [&](int k0, int kxn) {
    if (a.span) {
      const int total = (WG_TM - 1) * a.S + kxn;
      const long base = m0 * a.S + k0;
      for (int p = tid; p < total; p += 256) {
        const long o = base + p;
        xs[wg_skew(p, 6)] = o <= x_last ? xr[o] : 0.f;
      }
    } else {
      for (int e = tid; e < WG_TM * WG_SIDE_KX; e += 256) {
        const int m = e / WG_SIDE_KX, kk = e % WG_SIDE_KX;
        const bool ok = m0 + m < a.frames && kk < kxn;
        xs[m * WG_SIDE_PITCH + kk] = ok ? xr[(m0 + m) * a.S + k0 + kk] : 0.f;
      }
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }

  const int a_row = (wid * 32 + li) * a.SL + lh;      // image position of this lane's frame at k = lh of the slice
  int kx_base = 0, kx_next = 0;
  fetch_b(0);
  for (int k0 = 0; k0 < a.K; k0 += WG_BK) {
    __syncthreads();                                   // the previous chunk's LDS reads are done
    if (k0 == kx_next) {
      stage_x(k0, min(a.KX, a.K - k0));
      kx_base = k0;
      kx_next = k0 + a.KX;
    }
    stash_b();
    __syncthreads();
    if (k0 + WG_BK < a.K) fetch_b(k0 + WG_BK);         // in flight while this chunk computes
    const int pa = a_row + (k0 - kx_base);
    const int kleft = a.K - k0 - lh;                   // this lane's k of step ks is valid while 2 ks < kleft
#pragma unroll
    for (int ks = 0; ks < WG_BK / 2; ++ks) {
      float av = xs[wg_skew(pa + 2 * ks, sh)];
      av = 2 * ks < kleft ? av : 0.f;
      const float b0 = Bs[(2 * ks + lh) * WG_TN + li];
      const float b1 = Bs[(2 * ks + lh) * WG_TN + 32 + li];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
  }

  // C/D map of the 32 x 32 forms: column = lane & 31, row = (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5)
  float* __restrict__ orow = a.out + (size_t)r * a.out_row_stride;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const long m = m0 + wid * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
    if (m < a.frames) {
      const int j = j0 + li;
      if (j < a.N) orow[m * a.N + j] = acc0[v];
      if (j + 32 < a.N) orow[m * a.N + j + 32] = acc1[v];
    }
  }
}

}  // namespace
}  // namespace sda

using namespace sda;

extern "C" int sda_window_gemm_f32(const float* x, long x_row_stride, int rows, long frames, int S, int K, const float* B,
                                   int N, float* out, long out_row_stride, void* stream) {
  if (!x || !B || !out) { set_error("window_gemm: null argument"); return -1; }
  if (rows < 1 || frames < 1 || S < 1 || K < 1 || N < 1) { set_error("window_gemm: rows, frames, S, K and N must be positive"); return -1; }
  long need_x, need_out;
  if (__builtin_mul_overflow(frames - 1, (long)S, &need_x) || __builtin_add_overflow(need_x, (long)K, &need_x) ||
      __builtin_mul_overflow(frames, (long)N, &need_out)) {
    set_error("window_gemm: a row does not fit 63-bit indexing");
    return -1;
  }
  if (out_row_stride < need_out) { set_error("window_gemm: out_row_stride %ld < frames * N = %ld", out_row_stride, need_out); return -1; }
  if (x_row_stride < need_x) { set_error("window_gemm: x_row_stride %ld < (frames - 1) * S + K = %ld", x_row_stride, need_x); return -1; }
  WgArgs a;
  a.x = x; a.B = B; a.out = out;
  a.x_row_stride = x_row_stride; a.out_row_stride = out_row_stride; a.frames = frames;
  a.rows = rows; a.S = S; a.K = K; a.N = N;
  a.tiles_n = (N + WG_TN - 1) / WG_TN;
  a.tiles_m = (frames + WG_TM - 1) / WG_TM;
  long grid;
  if (__builtin_mul_overflow(a.tiles_m, (long)a.tiles_n, &grid) || __builtin_mul_overflow(grid, (long)rows, &grid) || grid > 0x7fffffffL) {
    set_error("window_gemm: grid too large");
    return -1;
  }
  // span form while the 127 frame strides plus one chunk of k, skewed, fit the image; KX = what is left, whole chunks
  const long lead = (long)(WG_TM - 1) * S;
  auto skewed = [](long n) { return n + (n >> 6) + 1; };
  if (skewed(lead + WG_BK) <= WG_XS) {
    long kx = (long)(K + WG_BK - 1) / WG_BK * WG_BK;
    while (skewed(lead + kx) > WG_XS) kx -= WG_BK;
    a.span = 1; a.SL = S; a.KX = (int)kx;
  } else {
    a.span = 0; a.SL = WG_SIDE_PITCH; a.KX = WG_SIDE_KX;
  }
  hipLaunchKernelGGL(window_gemm_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("window_gemm");
}
