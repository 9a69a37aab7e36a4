// lagged_cov — the lag products behind a time-lagged ridge regression (fp32, exact-fp32 MFMA):
//
//     out[s][d][i][j] = sum_{r in row slice s} a[r + d][i] * b[r][j]          d < L, i < Ap, j < Bp
//
// What it replaces: the accumulation of the normal equations of the backward mTRF, the field's linear decoding baseline
// (mne.decoding.TimeDelayingRidge with edge_correction=False: the autocorrelation method).  With a = b = x it gives the blocks
// A_d of the block-Toeplitz Gram matrix, with a = x, b = y the cross products R_l (speech_decoding_amd/ridge.py).
//
// Lag layout.  Both operands are rows of channels (channels-last, the channel count padded to 64, pad channels zero); sample n
// of (B, C, T) owns rows n (T + H) ... n (T + H) + T - 1 and H >= L - 1 zero rows follow it.  A lagged row that leaves its sample
// then lands in zeros, so the contraction runs over the flat row space without any per-sample masking.  Rows >= `rows` are never
// read and count as zero (the largest lags of the last sample's last rows).
//
// One workgroup = 4 waves owns a 64 x 64 tile of (i, j), a group of 8 consecutive lags and one slice of the rows; wave w owns the
// 32 x 32 quadrant (w & 1, w >> 1) of the tile for all 8 lags: 8 accumulators of v_mfma_f32_32x32x2_f32 = 128 registers.  The
// instruction's k is the row: lane l supplies A[i = l & 31][k = l >> 5] = a[r + k + d][i] and B[k = l >> 5][j = l & 31] =
// b[r + k][j], so both operands are lane-contiguous along the channel and every LDS read is 32 consecutive words per half wave:
// no bank is hit twice, whatever the pitch.  Per chunk of 64 rows the workgroup stages 64 + 7 rows of a's tile and 64 rows of
// b's once (global -> registers while the previous chunk computes -> LDS) and every lag of the group reads them: one b read and
// 8 a reads per 8 MFMAs.  b's rows past the slice end are staged as zeros, which ends the slice for every lag; a's are read on
// (a lagged row belongs to the slice of its b row).
//
// The number of slices depends on the shape alone (sda_lagged_cov_slices); each writes its own slab and the caller sums the
// slabs in fixed order.  No atomics; per output a k-ordered fmaf chain over the slice's rows: the same bits on every call.
#include "sd_common.h"

namespace sda {

namespace {

constexpr int LC_T = 64;                       // tile edge (channels of a x channels of b)
constexpr int LC_G = 8;                        // lags per workgroup
constexpr int LC_CH = 64;                      // rows per staged chunk
constexpr int LC_AROWS = LC_CH + LC_G - 1;     // rows of a per chunk
constexpr int LC_A4 = LC_AROWS * LC_T / 4;     // float4 pieces of a's image (1136)
constexpr int LC_B4 = LC_CH * LC_T / 4;        // ... and of b's (1024)
constexpr int LC_AE = (LC_A4 + 255) / 256;     // pieces per thread
constexpr int LC_BE = LC_B4 / 256;
constexpr long LC_MIN_SLICE = 256;             // rows: a slice is at least four chunks
constexpr long LC_TARGET_WGS = 1024;           // workgroups the slices fill the grid up to (two per CU, two rounds)

struct LcArgs {
  const float* a;
  const float* b;
  float* out;
  long a_pitch, b_pitch, rows, slice_len;
  int L, Ap, Bp;
  int tiles_a, tiles_b, groups;
};

// The workgroup's work for a group of NL lags (NL = 8 but for the last group of an L that is no multiple of 8).  NL is a template
// argument so that every MFMA of the loop is unconditional and the accumulators never change registers.
template <int NL>
__device__ __forceinline__ void lc_run(const LcArgs& p, float* __restrict__ as, float* __restrict__ bs, int i0, int j0, int d0, long s) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const long r_begin = s * p.slice_len;
  const long r_end = min(p.rows, r_begin + p.slice_len);

  // piece e of this thread: row (tid + 256 e) >> 4 of the image, channels 4 * (tid & 15) ... + 3
  // (a row outside the operand is never read: the load goes to the last row instead and the piece is zeroed)
  const float* __restrict__ ga = p.a + i0 + 4 * (tid & 15);
  const float* __restrict__ gb = p.b + j0 + 4 * (tid & 15);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra[LC_AE], rb[LC_BE];
  auto fetch = [&](long r0) {
#pragma unroll
    for (int e = 0; e < LC_AE; ++e) {
      const long row = r0 + d0 + ((tid + 256 * e) >> 4);
      const float4 v = load4(ga + (size_t)min(row, p.rows - 1) * p.a_pitch);
      ra[e] = row < p.rows ? v : zero4;
    }
#pragma unroll
    for (int e = 0; e < LC_BE; ++e) {
      const long row = r0 + ((tid + 256 * e) >> 4);
      const float4 v = load4(gb + (size_t)min(row, r_end - 1) * p.b_pitch);
      rb[e] = row < r_end ? v : zero4;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int e = 0; e < LC_AE; ++e) {
      const int idx = tid + 256 * e;
      if (idx < LC_A4) store4(as + 4 * idx, ra[e]);
    }
#pragma unroll
    for (int e = 0; e < LC_BE; ++e) store4(bs + 4 * (tid + 256 * e), rb[e]);
  };

  f32x16 acc[NL];
#pragma unroll
  for (int d = 0; d < NL; ++d)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[d][v] = 0.f;

  const int ih = wid & 1, jh = wid >> 1;
  const float* as_l = as + lh * LC_T + ih * 32 + li;      // this lane's element of image row k = lh
  const float* bs_l = bs + lh * LC_T + jh * 32 + li;
  fetch(r_begin);
  for (long r0 = r_begin; r0 < r_end; r0 += LC_CH) {
    __syncthreads();                                       // the previous chunk's LDS reads are done
    stash();
    __syncthreads();
    if (r0 + LC_CH < r_end) fetch(r0 + LC_CH);             // in flight while this chunk computes
#pragma unroll 4
    for (int ks = 0; ks < LC_CH / 2; ++ks) {
      const float bv = bs_l[2 * ks * LC_T];
#pragma unroll
      for (int d = 0; d < NL; ++d) acc[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(as_l[(2 * ks + d) * LC_T], bv, acc[d], 0, 0, 0);
    }
  }

  // C/D map of the 32 x 32 forms: column = lane & 31, row = (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5)
  float* __restrict__ o = p.out + ((size_t)s * p.L + d0) * p.Ap * p.Bp + (size_t)(i0 + ih * 32) * p.Bp + j0 + jh * 32 + li;
#pragma unroll
  for (int d = 0; d < NL; ++d) {
#pragma unroll
    for (int v = 0; v < 16; ++v) o[(size_t)((v & 3) + 8 * (v >> 2) + 4 * lh) * p.Bp] = acc[d][v];
    o += (size_t)p.Ap * p.Bp;
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void lagged_cov_kernel(const LcArgs p) {
  __shared__ __attribute__((aligned(16))) float as[LC_AROWS * LC_T];
  __shared__ __attribute__((aligned(16))) float bs[LC_CH * LC_T];
  long bid = blockIdx.x;
  const int it = (int)(bid % p.tiles_a);
  bid /= p.tiles_a;
  const int jt = (int)(bid % p.tiles_b);
  bid /= p.tiles_b;
  const int g = (int)(bid % p.groups);
  const long s = bid / p.groups;
  const int i0 = it * LC_T, j0 = jt * LC_T, d0 = g * LC_G;
  switch (min(LC_G, p.L - d0)) {                           // workgroup-uniform
    case 8: lc_run<8>(p, as, bs, i0, j0, d0, s); break;
    case 7: lc_run<7>(p, as, bs, i0, j0, d0, s); break;
    case 6: lc_run<6>(p, as, bs, i0, j0, d0, s); break;
    case 5: lc_run<5>(p, as, bs, i0, j0, d0, s); break;
    case 4: lc_run<4>(p, as, bs, i0, j0, d0, s); break;
    case 3: lc_run<3>(p, as, bs, i0, j0, d0, s); break;
    case 2: lc_run<2>(p, as, bs, i0, j0, d0, s); break;
    default: lc_run<1>(p, as, bs, i0, j0, d0, s); break;
  }
}

// slice length (a multiple of the chunk) and count for `rows` rows and `units` workgroups per slice
long lc_slices(long rows, long units, long* slice_len) {
  const long by_rows = (rows + LC_MIN_SLICE - 1) / LC_MIN_SLICE;
  long n = (LC_TARGET_WGS + units - 1) / units;
  n = n < 1 ? 1 : (n > by_rows ? by_rows : n);
  const long len = ((rows + n - 1) / n + LC_CH - 1) / LC_CH * LC_CH;
  *slice_len = len;
  return (rows + len - 1) / len;
}

bool lc_shape(long rows, int L, int Ap, int Bp, long* units) {
  if (rows < 1 || L < 1 || Ap < 1 || Bp < 1) { set_error("lagged_cov: rows, L, Ap and Bp must be positive"); return false; }
  if (Ap % LC_T || Bp % LC_T) { set_error("lagged_cov: Ap = %d and Bp = %d must be multiples of %d", Ap, Bp, LC_T); return false; }
  *units = (long)(Ap / LC_T) * (Bp / LC_T) * ((L + LC_G - 1) / LC_G);
  return true;
}

}  // namespace
}  // namespace sda

using namespace sda;

extern "C" int sda_lagged_cov_slices(long rows, int L, int Ap, int Bp) {
  long units, len;
  if (!lc_shape(rows, L, Ap, Bp, &units)) return -1;
  const long n = lc_slices(rows, units, &len);
  if (n > 0x7fffffffL) { set_error("lagged_cov: too many slices"); return -1; }
  return (int)n;
}

extern "C" long sda_lagged_cov_scratch_floats(long rows, int L, int Ap, int Bp) {
  const int n = sda_lagged_cov_slices(rows, L, Ap, Bp);
  long per, total;
  if (n < 0) return -1;
  if (__builtin_mul_overflow((long)L * Ap, (long)Bp, &per) || __builtin_mul_overflow(per, (long)n, &total)) {
    set_error("lagged_cov: the slabs do not fit 63-bit indexing");
    return -1;
  }
  return total;
}

extern "C" int sda_lagged_cov_f32(const float* a, long a_pitch, const float* b, long b_pitch, long rows, int L, int H, int Ap,
                                  int Bp, float* out, void* stream) {
  if (!a || !b || !out) { set_error("lagged_cov: null argument"); return -1; }
  long units;
  if (!lc_shape(rows, L, Ap, Bp, &units)) return -1;
  if (a_pitch < Ap || b_pitch < Bp) { set_error("lagged_cov: pitch a_pitch = %ld < Ap = %d or b_pitch = %ld < Bp = %d", a_pitch, Ap, b_pitch, Bp); return -1; }
  if (L - 1 > H) { set_error("lagged_cov: L - 1 = %d lags reach past the H = %d zero rows behind a sample", L - 1, H); return -1; }
  if (a_pitch % 4 || b_pitch % 4 || ((uintptr_t)a | (uintptr_t)b) % 16 || (uintptr_t)out % 4) {
    set_error("lagged_cov: operands must be 16-byte aligned with pitches that are multiples of 4 floats");
    return -1;
  }
  long need;
  if (sda_lagged_cov_scratch_floats(rows, L, Ap, Bp) < 0 || __builtin_mul_overflow(rows, a_pitch > b_pitch ? a_pitch : b_pitch, &need)) {
    set_error("lagged_cov: the operands do not fit 63-bit indexing");
    return -1;
  }
  LcArgs p;
  p.a = a; p.b = b; p.out = out;
  p.a_pitch = a_pitch; p.b_pitch = b_pitch; p.rows = rows;
  p.L = L; p.Ap = Ap; p.Bp = Bp;
  p.tiles_a = Ap / LC_T; p.tiles_b = Bp / LC_T; p.groups = (L + LC_G - 1) / LC_G;
  const long slices = lc_slices(rows, units, &p.slice_len);
  long grid;
  if (__builtin_mul_overflow(units, slices, &grid) || grid > 0x7fffffffL) { set_error("lagged_cov: grid too large"); return -1; }
  hipLaunchKernelGGL(lagged_cov_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("lagged_cov");
}
