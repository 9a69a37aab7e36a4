// stft_fft — the STFT of the log-mel path as a power-of-two FFT (fp32), the alternative to the window x DFT matrix on
// sda_window_gemm_f32 (n_fft * 2 n_freqs multiply-adds per frame there, a few thousand here):
//
//     X[r][m][b] = sum_{k < N} window[k] * x[r][m * hop + k] * exp(-2 pi i b k / N)            N = n_fft, b <= N / 2
//     out[r][m * out_pitch + 2 b] = Re X,   out[r][m * out_pitch + 2 b + 1] = Im X
//
// — the layout the window GEMM leaves and sda_mel_power_f32 reads.
//
// Factorisation.  A real frame y = window * x of N samples is the complex sequence z[k] = y[2 k] + i y[2 k + 1] of H = N / 2
// points.  Z = DFT_H(z) is computed by Stockham autosort passes (decimation in frequency: no separate digit-reversal pass — every
// pass writes its outputs where the next one reads them, and the last leaves natural order): radix-4 passes at strides
// s = 1, 4, 16, ..., and one closing radix-2 pass (no twiddles) when log2 H is odd.  A radix-4 pass at stride s, for
// t = q + s p (q < s, p < H / (4 s)), reads  a, b, c, d = src[t + k H / 4], k = 0 ... 3,  and writes
//     dst[q + 4 s p + s k] = w^(k p) (a + (-i)^k b + (-1)^k c + i^k d),      w = exp(-2 pi i s / H).
// Every twiddle w^(k p) = exp(-2 pi i (2 k p s) / N) is ONE entry of the caller's table twiddle[j] = exp(-2 pi i j / N), j < N / 2
// (j = 2 k p s < 3 N / 4; the entries at j >= N / 2 are the negated entries at j - N / 2) — correctly rounded values, never
// products of rounded values.  The split step then gives the one-sided spectrum: with E = (Z[b] + conj Z[H - b]) / 2 and
// O = (Z[b] - conj Z[H - b]) / (2 i),  X[b] = E + twiddle[b] O  for 0 < b < H,  X[0] = Re Z[0] + Im Z[0],  X[H] = Re Z[0] - Im Z[0];
// the imaginary parts of bins 0 and H are stored as exact zeros.  Multiplications by +-i, +-1 and 1 / 2 are exact; a complex
// product is two fmaf per component.
//
// One workgroup = 256 threads owns F = min(4096 / N, 32) consecutive frames of one row (N >= 128: F N / 8 = 512 radix-4
// butterflies per pass, 2 per thread).  Each frame lives in LDS as two planes (re, im); a pass works in place — every thread
// reads its butterflies into registers, the workgroup meets, then it writes them — so a workgroup holds one image of its
// frames: at most 29 KB with the twiddle table (23 KB at N = 512: six workgroups, 24 waves, per CU).
// x.  Lane = sample: a frame is read with consecutive dword loads at any alignment, times window[k], into plane k & 1 at
// k >> 1 (the plane pitch is 16 mod 32 words, so the two planes of one 32-lane write fall on different banks).  Frames that
// overlap (hop < N) read their samples again: from L2, the row is read from HBM once.
// LDS banks.  ds_read_b32 / ds_write_b32 bank 32-lane halves over 32 banks.  A pass READS t + k H / 4: consecutive lanes,
// consecutive words.  It WRITES q + 4 s p + s k: at s = 1, 4, 16 that strides 32 lanes over 128 words, so those buffers are
// kept skewed, word a at a + c (a >> 5) with c = 1, 4, 8 — each group of 32 words moved on by one run, conflict-free writes, and
// reads of 32 consecutive words stay inside one group.
// out.  Lane = float of the frame (2 b + re / im): each thread computes its own float from Z[b], Z[H - b] — 2 n_freqs consecutive
// dword stores per frame, coalesced at any alignment of out and out_pitch, and exactly those floats are written.
// Fixed operation order, no atomics: the same bits on every call.
#include "sd_common.h"

namespace sda {

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_SAMPLES = 4096;         // a workgroup owns F = min(SF_SAMPLES / n_fft, SF_MAX_FRAMES) frames (mirrored by
constexpr int SF_MAX_FRAMES = 32;        // ops.stft_fft_frames_per_workgroup)
__host__ __device__ constexpr int sf_frames(int N) { return SF_SAMPLES / N < SF_MAX_FRAMES ? SF_SAMPLES / N : SF_MAX_FRAMES; }

struct SfArgs {
  const float* x;
  const float* window;
  const float* twiddle;
  float* out;
  long x_row_stride, out_row_stride, out_pitch, frames, tiles_m;
  int hop;
};

// the skew of a buffer WRITTEN by a radix-4 pass at stride s
__host__ __device__ constexpr int sf_skew(int s) { return s == 1 ? 1 : (s == 4 ? 4 : (s == 16 ? 8 : 0)); }
__device__ __forceinline__ int sf_at(int a, int c) { return a + c * (a >> 5); }

template <int N>
__global__ __launch_bounds__(SF_THREADS) void stft_fft_kernel(const SfArgs a) {
  constexpr int H = N / 2, Q = H / 4, F = sf_frames(N);
  constexpr int PP = (H + H / 4 + 31) / 32 * 32 + 16;      // plane pitch: room for a skew of 8, and 16 mod 32
  static_assert(N >= 32 && N <= 2048 && (N & (N - 1)) == 0, "n_fft: a power of two in 32 ... 2048");
  static_assert(PP % 32 == 16, "the two planes of one write must fall on different banks");
  constexpr int IT4 = (F * Q + SF_THREADS - 1) / SF_THREADS, IT2 = (F * (H / 2) + SF_THREADS - 1) / SF_THREADS;
  __shared__ float Zs[F][2][PP];
  __shared__ float Tw[2][H];                         // twiddle[j] = (Tw[0][j], Tw[1][j]), j < N / 2
  const int tid = threadIdx.x;
  const long mt = (long)blockIdx.x % a.tiles_m;
  const int r = (int)((long)blockIdx.x / a.tiles_m);
  const long m0 = mt * F;
  const float* __restrict__ xr = a.x + (size_t)r * a.x_row_stride;

  for (int i = tid; i < N; i += SF_THREADS) Tw[i & 1][i >> 1] = a.twiddle[i];
  // a thread's samples sit at the same k in every frame: its window values are loaded once
  if constexpr (N >= SF_THREADS) {
    constexpr int KP = N / SF_THREADS;
    float wv[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) wv[j] = a.window[tid + j * SF_THREADS];
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const long m = m0 + f;
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        const int k = tid + j * SF_THREADS;
        Zs[f][k & 1][k >> 1] = m < a.frames ? xr[m * a.hop + k] * wv[j] : 0.f;
      }
    }
  } else {
    const int k = tid % N;
    const float wv = a.window[k];
#pragma unroll 8
    for (int f = tid / N; f < F; f += SF_THREADS / N) {
      const long m = m0 + f;
      Zs[f][k & 1][k >> 1] = m < a.frames ? xr[m * a.hop + k] * wv : 0.f;
    }
  }
  __syncthreads();

  // every pass works in place: all of a thread's butterflies are read, the workgroup meets, then they are written
  int c_src = 0;
#pragma unroll
  for (int s = 1; 4 * s <= H; s *= 4) {
    const int c_dst = sf_skew(s);
    float in[IT4][8];
#pragma unroll
    for (int e = 0; e < IT4; ++e) {
      const int i = tid + e * SF_THREADS;
      if (i < F * Q) {
        const int f = i / Q, t = i % Q;
        const float* zr = Zs[f][0];
        const float* zi = Zs[f][1];
        const int i0 = sf_at(t, c_src), i1 = sf_at(t + Q, c_src), i2 = sf_at(t + 2 * Q, c_src), i3 = sf_at(t + 3 * Q, c_src);
        in[e][0] = zr[i0]; in[e][1] = zi[i0]; in[e][2] = zr[i1]; in[e][3] = zi[i1];
        in[e][4] = zr[i2]; in[e][5] = zi[i2]; in[e][6] = zr[i3]; in[e][7] = zi[i3];
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < IT4; ++e) {
      const int i = tid + e * SF_THREADS;
      if (i >= F * Q) break;
      const int f = i / Q, t = i % Q;
      const int ps = t & ~(s - 1), q = t & (s - 1);
      const float ar = in[e][0], ai = in[e][1], br = in[e][2], bi = in[e][3], cr = in[e][4], ci = in[e][5], dr = in[e][6], di = in[e][7];
      const float pr = ar + cr, pi = ai + ci, mr = ar - cr, mi = ai - ci;       // a + c, a - c
      const float sr = br + dr, si = bi + di, tr = br - dr, ti = bi - di;       // b + d, b - d
      const float y1r = mr + ti, y1i = mi - tr;                                 // (a - c) - i (b - d)
      const float y2r = pr - sr, y2i = pi - si;
      const float y3r = mr - ti, y3i = mi + tr;                                 // (a - c) + i (b - d)
      const int j1 = 2 * ps, j2 = 4 * ps, j3 = 6 * ps;                          // j1 < N / 4, j2 < N / 2, j3 < 3 N / 4
      const float w1r = Tw[0][j1], w1i = Tw[1][j1], w2r = Tw[0][j2], w2i = Tw[1][j2];
      const bool wrap = j3 >= H;
      const float t3r = Tw[0][wrap ? j3 - H : j3], t3i = Tw[1][wrap ? j3 - H : j3];
      const float w3r = wrap ? -t3r : t3r, w3i = wrap ? -t3i : t3i;
      float* yr = Zs[f][0];
      float* yi = Zs[f][1];
      const int o = q + 4 * ps;
      const int o0 = sf_at(o, c_dst), o1 = sf_at(o + s, c_dst), o2 = sf_at(o + 2 * s, c_dst), o3 = sf_at(o + 3 * s, c_dst);
      yr[o0] = pr + sr;
      yi[o0] = pi + si;
      yr[o1] = __builtin_fmaf(y1r, w1r, -(y1i * w1i));
      yi[o1] = __builtin_fmaf(y1r, w1i, y1i * w1r);
      yr[o2] = __builtin_fmaf(y2r, w2r, -(y2i * w2i));
      yi[o2] = __builtin_fmaf(y2r, w2i, y2i * w2r);
      yr[o3] = __builtin_fmaf(y3r, w3r, -(y3i * w3i));
      yi[o3] = __builtin_fmaf(y3r, w3i, y3i * w3r);
    }
    __syncthreads();
    c_src = c_dst;
  }
  if constexpr ((__builtin_ctz(H) & 1) != 0) {       // log2 H odd: the closing radix-2 pass, stride H / 2, no twiddles
    float in[IT2][4];
#pragma unroll
    for (int e = 0; e < IT2; ++e) {
      const int i = tid + e * SF_THREADS;
      if (i < F * (H / 2)) {
        const int f = i / (H / 2), q = i % (H / 2);
        const int i0 = sf_at(q, c_src), i1 = sf_at(q + H / 2, c_src);
        in[e][0] = Zs[f][0][i0]; in[e][1] = Zs[f][1][i0]; in[e][2] = Zs[f][0][i1]; in[e][3] = Zs[f][1][i1];
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < IT2; ++e) {
      const int i = tid + e * SF_THREADS;
      if (i >= F * (H / 2)) break;
      const int f = i / (H / 2), q = i % (H / 2);
      Zs[f][0][q] = in[e][0] + in[e][2];
      Zs[f][1][q] = in[e][1] + in[e][3];
      Zs[f][0][q + H / 2] = in[e][0] - in[e][2];
      Zs[f][1][q + H / 2] = in[e][1] - in[e][3];
    }
    __syncthreads();
    c_src = 0;
  }

  // split step and store: element e = 2 b + (0: re, 1: im) of frame f
  float* __restrict__ orow = a.out + (size_t)r * a.out_row_stride;
  for (int i = tid; i < F * (N + 2); i += SF_THREADS) {
    const int f = i / (N + 2), e = i % (N + 2);
    const long m = m0 + f;
    if (m >= a.frames) break;                        // f grows with i: nothing further of this thread is in range
    const int b = e >> 1, bw = b & (H - 1);          // bins 0 and H both read Z[0]
    const int ib = sf_at(bw, c_src), ic = sf_at((H - b) & (H - 1), c_src);
    const float zr = Zs[f][0][ib], zi = Zs[f][1][ib], cr = Zs[f][0][ic], ci = Zs[f][1][ic];
    float v;
    if (b == 0 || b == H) {
      v = (e & 1) ? 0.f : (b == 0 ? zr + zi : zr - zi);
    } else {
      const float wr = Tw[0][bw], wi = Tw[1][bw];
      const float er = 0.5f * (zr + cr), ei = 0.5f * (zi - ci);                 // E
      const float pr = 0.5f * (zi + ci), pi = 0.5f * (cr - zr);                 // O
      v = (e & 1) ? __builtin_fmaf(wr, pi, __builtin_fmaf(wi, pr, ei)) : __builtin_fmaf(wr, pr, __builtin_fmaf(-wi, pi, er));
    }
    orow[m * a.out_pitch + e] = v;
  }
}

template <int N> void sf_launch(const SfArgs& a, unsigned grid, hipStream_t stream) {
  hipLaunchKernelGGL(stft_fft_kernel<N>, dim3(grid), dim3(SF_THREADS), 0, stream, a);
}

}  // namespace
}  // namespace sda

using namespace sda;

extern "C" int sda_stft_fft_f32(const float* x, long x_row_stride, int rows, long frames, int hop, int n_fft, const float* window,
                                const float* twiddle, float* out, long out_row_stride, long out_pitch, void* stream) {
  if (!x || !window || !twiddle || !out) { set_error("stft_fft: null argument"); return -1; }
  if (rows < 1 || frames < 1 || hop < 1 || n_fft < 1) { set_error("stft_fft: rows, frames, hop and n_fft must be positive"); return -1; }
  if (n_fft < 32 || n_fft > 2048 || (n_fft & (n_fft - 1)) != 0) {
    set_error("stft_fft: n_fft %d is not a power of two in 32 ... 2048", n_fft);
    return -1;
  }
  const long n_floats = n_fft + 2L;                  // 2 * n_freqs
  if (out_pitch < n_floats) { set_error("stft_fft: out_pitch %ld < 2 * n_freqs = %ld", out_pitch, n_floats); return -1; }
  long need_x, need_out;
  if (__builtin_mul_overflow(frames - 1, (long)hop, &need_x) || __builtin_add_overflow(need_x, (long)n_fft, &need_x) ||
      __builtin_mul_overflow(frames - 1, out_pitch, &need_out) || __builtin_add_overflow(need_out, n_floats, &need_out)) {
    set_error("stft_fft: a row does not fit 63-bit indexing");
    return -1;
  }
  if (out_row_stride < need_out) { set_error("stft_fft: out_row_stride %ld < (frames - 1) * out_pitch + 2 * n_freqs = %ld", out_row_stride, need_out); return -1; }
  if (x_row_stride < need_x) { set_error("stft_fft: x_row_stride %ld < (frames - 1) * hop + n_fft = %ld", x_row_stride, need_x); return -1; }
  long span_x, span_out;
  if (__builtin_mul_overflow((long)rows, x_row_stride, &span_x) || __builtin_mul_overflow((long)rows, out_row_stride, &span_out)) {
    set_error("stft_fft: the rows do not fit 63-bit indexing");
    return -1;
  }
  SfArgs a;
  a.x = x; a.window = window; a.twiddle = twiddle; a.out = out;
  a.x_row_stride = x_row_stride; a.out_row_stride = out_row_stride; a.out_pitch = out_pitch; a.frames = frames; a.hop = hop;
  const int F = sf_frames(n_fft);
  a.tiles_m = (frames + F - 1) / F;
  long grid;
  if (__builtin_mul_overflow(a.tiles_m, (long)rows, &grid) || grid > 0x7fffffffL) { set_error("stft_fft: grid too large"); return -1; }
  const hipStream_t st = (hipStream_t)stream;
  switch (n_fft) {
    case 32: sf_launch<32>(a, (unsigned)grid, st); break;
    case 64: sf_launch<64>(a, (unsigned)grid, st); break;
    case 128: sf_launch<128>(a, (unsigned)grid, st); break;
    case 256: sf_launch<256>(a, (unsigned)grid, st); break;
    case 512: sf_launch<512>(a, (unsigned)grid, st); break;
    case 1024: sf_launch<1024>(a, (unsigned)grid, st); break;
    default: sf_launch<2048>(a, (unsigned)grid, st); break;
  }
  return check_launch("stft_fft");
}
