// The encoder's gradient with respect to its input X (sda_input_grad):
//     dX[b][c][t] = sum_{d < Kp} W[w_b][d][c] * G[row(b, t)][d]          c < C, t < T
// G: the row-layout data gradient at the output of the SubjectBlock's first linear map (compute dtype, row pitch g_pitch);
// W: the (nW, Kp, Cp) matrix the forward applied, contracted over its ROW index — read as a transposed MFMA operand out of an
// LDS image (ds_read_b64_tr_b16 for the 16-bit types, tr_operand.h's fp32 path), so no transposed copy of the weights exists.
// Output: a contiguous (B, C, T) tensor of X's dtype, written from an LDS image of the tile: a wave stores 64 consecutive t.
#include "tr_operand.h"

namespace sda {
namespace {

constexpr int IG_TC = 64;            // input channels per workgroup tile (MFMA rows)
constexpr int IG_TT = 64;            // time steps per workgroup tile (MFMA columns)
constexpr int IG_KC = 32;            // contraction depth of one staged chunk
constexpr int IG_THREADS = 256;      // four waves, each a 32 x 32 quadrant of the tile

template <typename E> struct IgGeom {
  static constexpr int RB = IG_TC * (int)sizeof(E);                    // W image row (one d): 64 channels, swizzled chunks
  static constexpr int W_BYTES = IG_KC * RB;
  static constexpr int G_ROW = IG_KC * (int)sizeof(E);                 // G image row (one t): 32 d
  static constexpr int G_PITCH = G_ROW + 16;                           // padded: the operand reads of 16 rows spread over the banks
  static constexpr int G_BYTES = IG_TT * G_PITCH;
  static constexpr int W_PIECES = W_BYTES / 16 / IG_THREADS;           // 16-byte pieces per thread and chunk
  static constexpr int G_PIECES = IG_TT * G_ROW / 16 / IG_THREADS;
  static constexpr int OUT_BYTES = IG_TC * (IG_TT + 1) * 4;            // fp32 result tile, padded rows
  static constexpr int STAGE_BYTES = W_BYTES + G_BYTES;
  static constexpr int LDS = STAGE_BYTES > OUT_BYTES ? STAGE_BYTES : OUT_BYTES;
};

// second (non-transposed) operand: row t of the G image, the k values of mma16's lane-group convention
template <typename E> __device__ inline uint4 ig_g_operand(const unsigned char* row, int ks, int g);
template <> __device__ inline uint4 ig_g_operand<float>(const unsigned char* row, int ks, int g) {
  const float* p = reinterpret_cast<const float*>(row) + ks * 16 + g;
  return make_uint4(__float_as_uint(p[0]), __float_as_uint(p[4]), __float_as_uint(p[8]), __float_as_uint(p[12]));
}
template <typename E> __device__ inline uint4 ig_g_operand(const unsigned char* row, int ks, int g) {
  const uint2 lo = *reinterpret_cast<const uint2*>(row + (ks * 32 + 4 * g) * 2);
  const uint2 hi = *reinterpret_cast<const uint2*>(row + (ks * 32 + 16 + 4 * g) * 2);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

template <typename E> __device__ inline void ig_store(E* p, float v);
template <> __device__ inline void ig_store<float>(float* p, float v) { *p = v; }
template <> __device__ inline void ig_store<uint16_t>(uint16_t* p, float v) { *p = f2bf(v); }
template <> __device__ inline void ig_store<half_t>(half_t* p, float v) { *p = (half_t)v; }

struct IgArgs {
  const void* g;
  const void* w;
  const int* widx;
  void* out;
  long g_pitch;
  int nW, Kp, Cp, B, C, T;
};

// grid (C tiles, T tiles, B): the C tiles of one (b, t) tile are neighbours in launch order and share G's rows through L2
template <typename E, typename O>
__global__ __launch_bounds__(IG_THREADS) void input_grad_kernel(IgArgs a) {
  using Gm = IgGeom<E>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[Gm::LDS];
  unsigned char* wimg = smem;
  unsigned char* gimg = smem + Gm::W_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * IG_TC, t0 = blockIdx.y * IG_TT, b = blockIdx.z;
  int s = a.widx ? a.widx[b] : 0;
  s = (s < 0 || s >= a.nW) ? 0 : s;                                    // (the caller validated the indices: memory safety only)
  const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(a.w) + ((size_t)s * a.Kp * a.Cp + c0) * sizeof(E);
  const unsigned char* gsrc = reinterpret_cast<const unsigned char*>(a.g) +
                              ((size_t)b * rows_tp(a.T) + PAD + t0) * a.g_pitch * sizeof(E);

  // this thread's pieces of a chunk: (row, 16-byte chunk) of the W and G images, fixed for the whole K loop
  uint4 wv[Gm::W_PIECES], gv[Gm::G_PIECES];
  auto load = [&](int d0) {
#pragma unroll
    for (int i = 0; i < Gm::W_PIECES; ++i) {
      const int p = tid + i * IG_THREADS, r = p / (Gm::RB / 16), ch = p % (Gm::RB / 16);
      wv[i] = *reinterpret_cast<const uint4*>(wsrc + ((size_t)(d0 + r) * a.Cp) * sizeof(E) + ch * 16);
    }
#pragma unroll
    for (int i = 0; i < Gm::G_PIECES; ++i) {
      const int p = tid + i * IG_THREADS, r = p / (Gm::G_ROW / 16), ch = p % (Gm::G_ROW / 16);
      gv[i] = (t0 + r < a.T) ? *reinterpret_cast<const uint4*>(gsrc + (size_t)r * a.g_pitch * sizeof(E) + d0 * sizeof(E) + ch * 16)
                             : make_uint4(0, 0, 0, 0);
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int i = 0; i < Gm::W_PIECES; ++i) {
      const int p = tid + i * IG_THREADS, r = p / (Gm::RB / 16), ch = p % (Gm::RB / 16);
      *reinterpret_cast<uint4*>(wimg + r * Gm::RB + ((ch ^ chunk_xor<E, Gm::RB>(r)) << 4)) = wv[i];
    }
#pragma unroll
    for (int i = 0; i < Gm::G_PIECES; ++i) {
      const int p = tid + i * IG_THREADS, r = p / (Gm::G_ROW / 16), ch = p % (Gm::G_ROW / 16);
      *reinterpret_cast<uint4*>(gimg + r * Gm::G_PITCH + ch * 16) = gv[i];
    }
  };

  const int wm = wave & 1, wn = wave >> 1, g = lane >> 4, i16 = lane & 15;
  f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int KSTEP = sizeof(E) == 4 ? 16 : 32;                      // k values of one mma16
  const int nk = a.Kp / IG_KC;
  load(0);
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();                                                   // the previous chunk is consumed
    put();
    __syncthreads();
    if (kc + 1 < nk) load((kc + 1) * IG_KC);                           // next chunk's loads fly under this chunk's MFMAs
#pragma unroll
    for (int ks = 0; ks < IG_KC / KSTEP; ++ks) {
      uint4 af[2], bf[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) af[m] = TrOp<E, Gm::RB>::get(wimg, ks * KSTEP, wm * 32 + m * 16, lane);
#pragma unroll
      for (int n = 0; n < 2; ++n) bf[n] = ig_g_operand<E>(gimg + (wn * 32 + n * 16 + i16) * Gm::G_PITCH, ks, g);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = mma16<E>(af[m], bf[n], acc[m][n]);
    }
  }

  // result tile through LDS: lane l holds rows 4 (l >> 4) + v (channels), column l & 15 (time) of each 16 x 16 block
  __syncthreads();
  float* ot = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int v = 0; v < 4; ++v) ot[(wm * 32 + m * 16 + 4 * g + v) * (IG_TT + 1) + wn * 32 + n * 16 + i16] = acc[m][n][v];
  __syncthreads();
  O* out = reinterpret_cast<O*>(a.out);
  const int t = t0 + lane;
#pragma unroll 4
  for (int r = wave; r < IG_TC; r += IG_THREADS / 64) {
    const int c = c0 + r;
    if (c < a.C && t < a.T) ig_store<O>(out + ((size_t)b * a.C + c) * a.T + t, ot[r * (IG_TT + 1) + lane]);
  }
}

template <typename E, typename O>
void launch_input_grad(const IgArgs& a, hipStream_t st) {
  const dim3 grid((a.C + IG_TC - 1) / IG_TC, (a.T + IG_TT - 1) / IG_TT, a.B);
  hipLaunchKernelGGL((input_grad_kernel<E, O>), grid, dim3(IG_THREADS), 0, st, a);
}

template <typename E>
void dispatch_input_grad(int out_dtype, const IgArgs& a, hipStream_t st) {
  switch (out_dtype) {
    case SDA_F32: launch_input_grad<E, float>(a, st); break;
    case SDA_BF16: launch_input_grad<E, uint16_t>(a, st); break;
    default: launch_input_grad<E, half_t>(a, st); break;
  }
}

bool ig_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace sda

extern "C" int sda_input_grad(const void* g, long g_pitch, const void* w, const int* widx, int nW, int Kp, int Cp, int B, int C,
                              int T, int dtype, void* out, int out_dtype, void* stream) {
  using namespace sda;
  if (!g || !w || !out) { set_error("input_grad: null G, W or output"); return -1; }
  if (dtype != SDA_F32 && dtype != SDA_BF16 && dtype != SDA_F16) { set_error("input_grad: unknown dtype %d", dtype); return -1; }
  if (out_dtype != SDA_F32 && out_dtype != SDA_BF16 && out_dtype != SDA_F16) {
    set_error("input_grad: unknown output dtype %d", out_dtype);
    return -1;
  }
  if (B < 1 || C < 1 || T < 1 || nW < 1 || B > 65535 || T > 65535 * IG_TT) {
    set_error("input_grad: bad sizes (B %d, C %d, T %d, nW %d)", B, C, T, nW);
    return -1;
  }
  if (Kp < IG_KC || Kp % IG_KC || Cp < C || Cp % SDA_CH_ALIGN || g_pitch < Kp || g_pitch % 8) {
    set_error("input_grad: W must be (nW, Kp, Cp) with Kp a multiple of %d, Cp a multiple of %d and >= C, and G's pitch >= Kp "
              "(got Kp %d, Cp %d, C %d, pitch %ld)", IG_KC, SDA_CH_ALIGN, Kp, Cp, C, g_pitch);
    return -1;
  }
  if (!ig_aligned16(g) || !ig_aligned16(w)) { set_error("input_grad: G and W must be 16-byte aligned"); return -1; }
  if (nW > 1 && !widx) { set_error("input_grad: %d matrices need per-sample indices", nW); return -1; }
  IgArgs a{g, w, widx, out, g_pitch, nW, Kp, Cp, B, C, T};
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case SDA_F32: dispatch_input_grad<float>(out_dtype, a, st); break;
    case SDA_BF16: dispatch_input_grad<uint16_t>(out_dtype, a, st); break;
    default: dispatch_input_grad<half_t>(out_dtype, a, st); break;
  }
  return check_launch("input_grad");
}
