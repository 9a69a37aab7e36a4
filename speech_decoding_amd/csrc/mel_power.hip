// mel_power — the pass behind the STFT window GEMM: power spectrum, mel filterbank, log compression (fp32, exact-fp32 MFMA):
//
//     P[r][m][b]   = spec[r][m * spec_pitch + 2 b]^2 + spec[r][m * spec_pitch + 2 b + 1]^2              b < n_freqs
//     mel[r][j][m] = sum_{b < n_freqs} P[r][m][b] * fb[b * n_mels + j]                                  j < n_mels, m < frames
//     out[r][j * out_pitch + m] = log_eps < 0 ? mel : logf(log_eps + mel)
//
// What it replaces: torchaudio.transforms.MelSpectrogram(power=2.0) behind its STFT, and the log(eps + mel) of the paper's
// "Deep Mel" / regression baselines.  The STFT itself is sda_window_gemm_f32 with S = hop, K = n_fft, N = 2 * n_freqs
// (signal_prep.stft); its output, frames x (re, im) interleaved, is this kernel's `spec` as it stands.
//
// One workgroup = 4 waves owns 128 consecutive frames of one row x 32 * NC mel columns (NC = 1, 2 or 4 by n_mels: up to 128,
// so the paper's 120 columns read the spectrum once); wave w owns frames [32 w, 32 w + 32) on the M index of
// v_mfma_f32_32x32x2_f32 (lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]) and keeps NC independent
// 32 x 32 accumulators, so one A fragment feeds NC MFMAs.  The contraction runs in chunks of 32 bins:
//
// spec.  A frame's chunk is 64 consecutive floats: one wave reads it with one coalesced 256-byte load (lane = float, so no
// alignment of spec or spec_pitch is needed), 32 frames per wave and chunk, global -> registers while the previous chunk
// computes.  The lane pair (re, im) meets through one DPP swap, P = fmaf(im, im, re * re) goes to LDS as [frame][parity][bin / 2]
// at a pitch of 36 words: lane (i, k) of the A fragment needs the bins 2 ks + k, ks = 0 ... 15 — 16 consecutive words, four
// 16-byte reads per chunk, and 36 i runs through all sixteen 4-bank groups.
// fb.  Constant and L2-resident (123 kB at the paper's setting); streamed like window_gemm's B: 32 rows x 32 NC columns per
// chunk, global -> registers -> LDS, the columns permuted (column 32 c + i at word NC i + c) so that lane (i, k) reads the B
// values of all NC accumulators of one MFMA step with one 4 NC-byte read.
// Out-of-range elements — bins b >= n_freqs (the odd tail: 257 = 8 * 32 + 1), columns j >= n_mels, frames m >= frames — are
// loaded from the nearest valid address and replaced by zero on their way to LDS (no branch around a load, and nothing outside
// the contract is read); they are zero in BOTH images, so no padding value meets a NaN.
// Epilogue.  One accumulator at a time is transposed through LDS ([column][frame], the C/D registers' four consecutive
// frames as one 16-byte write), then read back with consecutive lanes along m, the log applied, and stored as 512-byte runs
// of out[r][j][m0 ...]: dword stores, coalesced at any alignment of out and out_pitch; ragged frame / column edges are masked
// at the store.  Results are a b-ordered fmaf chain per output: bitwise reproducible, no atomics.
#include "sd_common.h"

namespace sda {

namespace {

constexpr int MP_TM = 128;               // frames per workgroup (32 per wave)
constexpr int MP_BK = 32;                // bins per chunk
constexpr int MP_PP = 36;                // pitch of the power image [frame][parity of the bin][bin / 2] (16-byte rows)
constexpr int MP_FP = 132;               // pitch of the filterbank chunk [bin][permuted column] (16-byte rows)
constexpr int MP_TP = 132;               // pitch of the transposed accumulator [column][frame] (16-byte rows)

struct MpArgs {
  const float* spec;
  const float* fb;
  float* out;
  long spec_row_stride, spec_pitch, out_row_stride, out_pitch, frames;
  int rows, n_freqs, n_mels;
  int tiles_n;
  long tiles_m;
  float log_eps;
};

template <int NC>
__global__ __launch_bounds__(256, 2) void mel_power_kernel(const MpArgs a) {
  __shared__ __attribute__((aligned(16))) float Ps[MP_TM * MP_PP];
  __shared__ __attribute__((aligned(16))) float Fs[MP_BK * MP_FP];     // the epilogue's transposed accumulator lives here too
  static_assert(32 * MP_TP <= MP_BK * MP_FP, "the transposed accumulator must fit the filterbank chunk");
  constexpr int TN = 32 * NC;
  struct alignas(4 * NC) bvec { float v[NC]; };                       // one 4 NC-byte LDS read
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);           // scalar: a frame's address is a scalar base + lane
  const int li = lane & 31, lh = lane >> 5;
  long bid = blockIdx.x;
  const int nt = (int)(bid % a.tiles_n);
  bid /= a.tiles_n;
  const long mt = bid % a.tiles_m;
  const int r = (int)(bid / a.tiles_m);
  const long m0 = mt * MP_TM;
  const int j0 = nt * TN;
  const float* __restrict__ sr = a.spec + (size_t)r * a.spec_row_stride;
  const int n_floats = 2 * a.n_freqs;                                  // of a frame

  // spec chunk: element e of this thread = float `lane` of frame wid + 4 e of the tile
  float rs[MP_TM / 4];
  auto fetch_s = [&](int b0) {
    const int f = min(2 * b0 + lane, n_floats - 1);
#pragma unroll
    for (int e = 0; e < MP_TM / 4; ++e) rs[e] = sr[min(m0 + wid + 4 * e, a.frames - 1) * a.spec_pitch + f];
  };
  const int p_word = (lane >> 1 & 1) * 16 + (lane >> 2);               // bin lane / 2 of the chunk: [parity][half]
  auto stash_s = [&](int b0) {
    const bool f_ok = 2 * b0 + lane < n_floats;
#pragma unroll
    for (int e = 0; e < MP_TM / 4; ++e) {
      const float v = (f_ok && m0 + wid + 4 * e < a.frames) ? rs[e] : 0.f;
      // lanes 2 b, 2 b + 1 swap (DPP quad_perm [1, 0, 3, 2]): the even lane holds re and receives im
      const float other = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));
      if (!(lane & 1)) Ps[(wid + 4 * e) * MP_PP + p_word] = __builtin_fmaf(other, other, v * v);
    }
  };
  // fb chunk: element e of this thread = flat index tid + 256 e of the 32 x TN chunk (coalesced along j); 256 % TN == 0, so
  // the column is the same for every e
  const int bj = tid % TN;
  const bool j_ok = j0 + bj < a.n_mels;
  const float* __restrict__ fcol = a.fb + min(j0 + bj, a.n_mels - 1);
  const int f_word = (tid / TN) * MP_FP + (bj & 31) * NC + (bj >> 5);
  float rb[4 * NC];
  auto fetch_b = [&](int b0) {
#pragma unroll
    for (int e = 0; e < 4 * NC; ++e) rb[e] = fcol[(size_t)min(b0 + tid / TN + (256 / TN) * e, a.n_freqs - 1) * a.n_mels];
  };
  auto stash_b = [&](int b0) {
#pragma unroll
    for (int e = 0; e < 4 * NC; ++e)
      Fs[f_word + (256 / TN) * e * MP_FP] = (j_ok && b0 + tid / TN + (256 / TN) * e < a.n_freqs) ? rb[e] : 0.f;
  };

  f32x16 acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[c][v] = 0.f;

  const float* pa = &Ps[(wid * 32 + li) * MP_PP + lh * 16];            // this lane's frame, the bins of parity lh
  const float* pb = &Fs[lh * MP_FP + li * NC];                         // row lh of an MFMA step, this lane's NC columns
  fetch_s(0);
  fetch_b(0);
  for (int b0 = 0; b0 < a.n_freqs; b0 += MP_BK) {
    __syncthreads();                                 // the previous chunk's LDS reads are done
    stash_s(b0);
    stash_b(b0);
    __syncthreads();
    if (b0 + MP_BK < a.n_freqs) {                    // in flight while this chunk computes
      fetch_s(b0 + MP_BK);
      fetch_b(b0 + MP_BK);
    }
    f32x4 av[4];
    bvec bv[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) av[q] = *reinterpret_cast<const f32x4*>(pa + 4 * q);
#pragma unroll
    for (int t = 0; t < 4; ++t) bv[0][t] = *reinterpret_cast<const bvec*>(pb + 2 * t * MP_FP);
#pragma unroll
    for (int q = 0; q < 4; ++q) {                    // MFMA steps ks = 4 q + t; the next four steps' B on its way meanwhile
      if (q < 3) {
#pragma unroll
        for (int t = 0; t < 4; ++t) bv[(q + 1) & 1][t] = *reinterpret_cast<const bvec*>(pb + 2 * (4 * (q + 1) + t) * MP_FP);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][t], bv[q & 1][t].v[c], acc[c], 0, 0, 0);
    }
  }

  // C/D map of the 32 x 32 forms: column = lane & 31, row = (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5)
  float* __restrict__ orow = a.out + (size_t)r * a.out_row_stride;
  const bool take_log = !(a.log_eps < 0.f);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (j0 + 32 * c >= a.n_mels) break;              // uniform over the workgroup
    __syncthreads();                                 // the last chunk's / the previous accumulator's LDS reads are done
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(&Fs[li * MP_TP + wid * 32 + 8 * g + 4 * lh]) =
          make_float4(acc[c][4 * g], acc[c][4 * g + 1], acc[c][4 * g + 2], acc[c][4 * g + 3]);
    __syncthreads();
    const long m = m0 + (tid & 127);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int jt = (tid >> 7) + 2 * e;
      const int j = j0 + 32 * c + jt;
      if (j < a.n_mels && m < a.frames) {
        float v = Fs[jt * MP_TP + (tid & 127)];
        if (take_log) v = logf(a.log_eps + v);
        orow[j * a.out_pitch + m] = v;
      }
    }
  }
}

}  // namespace
}  // namespace sda

using namespace sda;

extern "C" int sda_mel_power_f32(const float* spec, long spec_row_stride, long spec_pitch, int rows, long frames, int n_freqs,
                                 const float* fb, int n_mels, float log_eps, float* out, long out_row_stride, long out_pitch,
                                 void* stream) {
  if (!spec || !fb || !out) { set_error("mel_power: null argument"); return -1; }
  if (rows < 1 || frames < 1 || n_freqs < 1 || n_mels < 1) { set_error("mel_power: rows, frames, n_freqs and n_mels must be positive"); return -1; }
  if (n_freqs > 0x3fffffff) { set_error("mel_power: n_freqs too large"); return -1; }
  if (spec_pitch < 2L * n_freqs) { set_error("mel_power: spec_pitch %ld < 2 * n_freqs = %ld", spec_pitch, 2L * n_freqs); return -1; }
  if (out_pitch < frames) { set_error("mel_power: out_pitch %ld < frames = %ld", out_pitch, frames); return -1; }
  long need_spec, need_out;
  if (__builtin_mul_overflow(frames - 1, spec_pitch, &need_spec) || __builtin_add_overflow(need_spec, 2L * n_freqs, &need_spec) ||
      __builtin_mul_overflow((long)n_mels - 1, out_pitch, &need_out) || __builtin_add_overflow(need_out, frames, &need_out)) {
    set_error("mel_power: a row does not fit 63-bit indexing");
    return -1;
  }
  if (spec_row_stride < need_spec) { set_error("mel_power: spec_row_stride %ld < (frames - 1) * spec_pitch + 2 * n_freqs = %ld", spec_row_stride, need_spec); return -1; }
  if (out_row_stride < need_out) { set_error("mel_power: out_row_stride %ld < (n_mels - 1) * out_pitch + frames = %ld", out_row_stride, need_out); return -1; }
  const int NC = n_mels > 64 ? 4 : (n_mels > 32 ? 2 : 1);
  MpArgs a;
  a.spec = spec; a.fb = fb; a.out = out;
  a.spec_row_stride = spec_row_stride; a.spec_pitch = spec_pitch; a.out_row_stride = out_row_stride; a.out_pitch = out_pitch;
  a.frames = frames; a.rows = rows; a.n_freqs = n_freqs; a.n_mels = n_mels; a.log_eps = log_eps;
  a.tiles_n = (n_mels + 32 * NC - 1) / (32 * NC);
  a.tiles_m = (frames + MP_TM - 1) / MP_TM;
  long grid;
  if (__builtin_mul_overflow(a.tiles_m, (long)a.tiles_n, &grid) || __builtin_mul_overflow(grid, (long)rows, &grid) || grid > 0x7fffffffL) {
    set_error("mel_power: grid too large");
    return -1;
  }
  const dim3 g((unsigned)grid), b(256);
  if (NC == 4) hipLaunchKernelGGL(mel_power_kernel<4>, g, b, 0, (hipStream_t)stream, a);
  else if (NC == 2) hipLaunchKernelGGL(mel_power_kernel<2>, g, b, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(mel_power_kernel<1>, g, b, 0, (hipStream_t)stream, a);
  return check_launch("mel_power");
}
