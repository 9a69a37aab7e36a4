// Whole-recording input path of Brennan2018 (brennan2018.py:72-152): RobustScaler over the WHOLE recording per
// (subject, channel) row — or per channel with every subject pooled (preprocs.subject_wise = False) — then clamp, then
// segmentation, then baseline correction per segment.  Rows here are tens of thousands to millions of samples, not the 360
// one wavefront sorts in collate.hip, so the three order statistics are SELECTED, not sorted:
//
//   sda_robust_stats           radix select on order-preserving 32-bit keys, four 8-bit passes, most significant byte first.
//                              The six target ranks (floor and floor + 1 of the positions of q = 0.25, 0.5, 0.75) are resolved
//                              in the same passes: targets whose key prefixes agree so far share one histogram ("group").
//                              A pass = one counting launch (a row may be cut over many workgroups: 256-bin histograms in LDS,
//                              non-zero bins added to the row's histogram in global memory with integer atomics — integer adds
//                              commute, the counts are the same whatever the arrival order) + one resolving launch (one
//                              workgroup per row walks the bins, narrows every target, regroups, zeroes the histogram).
//                              Launch order on the stream is the only synchronisation between workgroups.
//   sda_scale_clamp_rows       y = (x - centre[row]) / scale[row], clamped: one streaming pass.
//   sda_gather_baseline_windows dst[b, c, :] = w - mean(w[:nb]), any T.
//
// A row is `n_chunks` pieces of `chunk_len` floats, `chunk_stride` apart; rows are `row_stride` apart:
//   subject-wise on X (S, C, L): rows = S * C, row_stride = L, one chunk;
//   pooled:                      rows = C, row_stride = L, S chunks, chunk_stride = C * L — no rearranging copy.
#include "sd_common.h"

namespace sda {

constexpr int RS_TARGETS = 6;            // ranks resolved per row
constexpr int RS_BINS = 256;             // 8-bit passes
constexpr int RS_STATE = 32;             // uint32 words of per-row state
constexpr int RS_WG_ELEMS = 4096;        // the smallest share of a row one workgroup counts
// per-row state words
constexpr int ST_RANK = 0;               // [6] rank of the target among the elements that match its prefix
constexpr int ST_PREFIX = 6;             // [6] key bits resolved so far (right-aligned)
constexpr int ST_GPREFIX = 12;           // [6] distinct prefixes = groups
constexpr int ST_GROUP = 18;             // [6] group of target k
constexpr int ST_NGROUPS = 24;

struct RankTable { unsigned rank[RS_TARGETS]; };

// float bits -> key with the same order as the floats (-inf lowest, +inf highest); -0.0 counts as +0.0
__device__ inline uint32_t order_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float key_value(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

__global__ __launch_bounds__(256) void robust_init_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ hist, long rows, RankTable ranks) {
  const long row = blockIdx.x;
  if (row >= rows) return;
  uint32_t* st = state + row * RS_STATE;
  uint32_t* h = hist + row * (RS_TARGETS * RS_BINS);
  for (int i = threadIdx.x; i < RS_TARGETS * RS_BINS; i += 256) h[i] = 0u;
  if (threadIdx.x < RS_STATE) {
    const int i = threadIdx.x;
    uint32_t v = 0u;
    if (i < ST_RANK + RS_TARGETS) v = ranks.rank[i];
    else if (i == ST_NGROUPS) v = 1u;
    st[i] = v;                                          // prefixes, group prefixes and group indices all start at 0
  }
}

// pass p (0 = most significant byte): every element whose resolved bits equal a group's prefix counts in that group's bin
__global__ __launch_bounds__(256) void robust_count_kernel(const float* __restrict__ x, long row_stride, int n_chunks, long chunk_len,
                                                           long chunk_stride, long share, const uint32_t* __restrict__ state,
                                                           uint32_t* __restrict__ hist, int pass) {
  __shared__ uint32_t lh[RS_TARGETS * RS_BINS];
  const long row = blockIdx.y;
  const uint32_t* st = state + row * RS_STATE;
  const int ngroups = min((int)st[ST_NGROUPS], RS_TARGETS);
  uint32_t gp[RS_TARGETS];
#pragma unroll
  for (int g = 0; g < RS_TARGETS; ++g) gp[g] = st[ST_GPREFIX + g];
  for (int i = threadIdx.x; i < ngroups * RS_BINS; i += 256) lh[i] = 0u;
  __syncthreads();
  const long N = (long)n_chunks * chunk_len;
  const long lo = (long)blockIdx.x * share, hi = min(N, lo + share);
  const int shift = 24 - 8 * pass;
  const float* base = x + row * row_stride;
  for (long c = lo / chunk_len; c < n_chunks && c * chunk_len < hi; ++c) {
    const long a = max(lo, c * chunk_len) - c * chunk_len, b = min(hi, (c + 1) * chunk_len) - c * chunk_len;
    const float* p = base + c * chunk_stride;
    for (long i = a + threadIdx.x; i < b; i += 256) {
      const uint32_t key = order_key(p[i]);
      const uint32_t bin = (key >> shift) & 255u;
      const uint32_t head = pass == 0 ? 0u : key >> (shift + 8);
#pragma unroll
      for (int g = 0; g < RS_TARGETS; ++g)
        if (g < ngroups && head == gp[g]) atomicAdd(&lh[g * RS_BINS + bin], 1u);
    }
  }
  __syncthreads();
  uint32_t* h = hist + row * (RS_TARGETS * RS_BINS);
  for (int i = threadIdx.x; i < ngroups * RS_BINS; i += 256) {
    const uint32_t v = lh[i];
    if (v) atomicAdd(&h[i], v);
  }
}

// one workgroup per row: narrow the six targets by the byte just counted, regroup, zero the histogram; after the last pass
// the prefixes ARE the selected keys: write centre and scale
__global__ __launch_bounds__(256) void robust_resolve_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ hist, long rows, int pass,
                                                             float g25, float g50, float g75, float* __restrict__ centre,
                                                             float* __restrict__ scale) {
  __shared__ uint32_t pre[RS_TARGETS], rnk[RS_TARGETS];
  const long row = blockIdx.x;
  if (row >= rows) return;
  uint32_t* st = state + row * RS_STATE;
  uint32_t* h = hist + row * (RS_TARGETS * RS_BINS);
  if (threadIdx.x < RS_TARGETS) {
    const int k = threadIdx.x;
    const int g = min((int)st[ST_GROUP + k], RS_TARGETS - 1);
    uint32_t r = st[ST_RANK + k];
    const uint32_t* hg = h + g * RS_BINS;
    int bin = RS_BINS - 1;                      // (a rank beyond the counted total cannot happen; the last bin bounds the walk)
    for (int i = 0; i < RS_BINS; ++i) {
      const uint32_t n = hg[i];
      if (r < n) { bin = i; break; }
      if (i < RS_BINS - 1) r -= n;
    }
    pre[k] = (st[ST_PREFIX + k] << 8) | (uint32_t)bin;
    rnk[k] = r;
  }
  __syncthreads();                               // every read of the histogram is done
  for (int i = threadIdx.x; i < RS_TARGETS * RS_BINS; i += 256) h[i] = 0u;
  if (threadIdx.x == 0) {
    int ng = 0;
    uint32_t gp[RS_TARGETS];
    for (int k = 0; k < RS_TARGETS; ++k) {
      int g = -1;
      for (int j = 0; j < ng; ++j)
        if (gp[j] == pre[k]) { g = j; break; }
      if (g < 0) { g = ng; gp[ng++] = pre[k]; }
      st[ST_RANK + k] = rnk[k];
      st[ST_PREFIX + k] = pre[k];
      st[ST_GROUP + k] = (uint32_t)g;
    }
    for (int j = 0; j < RS_TARGETS; ++j) st[ST_GPREFIX + j] = j < ng ? gp[j] : 0u;
    st[ST_NGROUPS] = (uint32_t)ng;
    if (pass == 3) {
      // numpy's "linear" rule (position and fraction computed in double by the caller): a + (b - a) * g; g == 0 takes the
      // element itself, so an infinite upper neighbour does not turn an exact position into NaN
      auto lerp = [&](int k, float g) {
        const float a = key_value(pre[k]), b = key_value(pre[k + 1]);
        return g == 0.f ? a : a + (b - a) * g;
      };
      const float med = lerp(2, g50);
      float iqr = lerp(4, g75) - lerp(0, g25);
      if (iqr == 0.f) iqr = 1.f;                 // sklearn _handle_zeros_in_scale
      centre[row] = med;
      scale[row] = iqr;
    }
  }
}

constexpr int SC_WG_ELEMS = 8192;        // elements of one chunk a workgroup of the streaming pass scales

__global__ __launch_bounds__(256) void scale_clamp_rows_kernel(const float* __restrict__ x, float* __restrict__ y, long row_stride, int n_chunks,
                                                               long chunk_len, long chunk_stride, int pieces, const float* __restrict__ centre,
                                                               const float* __restrict__ scale, float lim, int do_clamp) {
  const long bid = blockIdx.x;
  const long rc = bid / pieces;
  const int piece = (int)(bid % pieces);
  const long row = rc / n_chunks, chunk = rc % n_chunks;
  const long lo = (long)piece * SC_WG_ELEMS, hi = min(chunk_len, lo + SC_WG_ELEMS);
  if (lo >= hi) return;
  const float c = centre[row], s = scale[row];
  const long off = row * row_stride + chunk * chunk_stride + lo;
  const float* px = x + off;
  float* py = y + off;
  const long n = hi - lo;
  auto f = [&](float v) {
    float o = (v - c) / s;
    if (do_clamp) o = fminf(fmaxf(o, -lim), lim);
    return o;
  };
  // 16-byte accesses on the part of the piece where BOTH pointers are 16-byte aligned (they share `off`: in place always,
  // out of place when the two bases agree modulo 16), 4-byte accesses on the head and tail, or on all of it otherwise
  long head = n;
  if (((reinterpret_cast<uintptr_t>(px) ^ reinterpret_cast<uintptr_t>(py)) & 15) == 0)
    head = min(n, (long)(((16 - (reinterpret_cast<uintptr_t>(px) & 15)) & 15) >> 2));
  const long nvec = (n - head) / 4;
  for (long i = threadIdx.x; i < head; i += 256) py[i] = f(px[i]);
  for (long i = threadIdx.x; i < nvec; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(px + head + 4 * i);
    *reinterpret_cast<float4*>(py + head + 4 * i) = make_float4(f(v.x), f(v.y), f(v.z), f(v.w));
  }
  for (long i = head + 4 * nvec + threadIdx.x; i < n; i += 256) py[i] = f(px[i]);
}

// one wavefront per (sample, channel) row: the baseline sum runs in a fixed order (lane l adds samples l, l + 64, ... in
// order, then the butterfly), so the same window gives the same bits
__global__ __launch_bounds__(256) void gather_baseline_windows_kernel(const float* const* __restrict__ win_ptr, const long* __restrict__ win_cstride,
                                                                      float* __restrict__ dst, long rows, int C, int T, int nb) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  const long b = row / C, c = row % C;
  const float* w = win_ptr[b] + c * win_cstride[b];
  float bsum = 0.f;
  for (int t = lane; t < nb; t += 64) bsum += w[t];
  const float base = nb > 0 ? wave_sum(bsum) / (float)nb : 0.f;
  float* y = dst + row * T;
  for (int t = lane; t < T; t += 64) y[t] = w[t] - base;
}

}  // namespace sda

using namespace sda;

static bool bad_rows(long rows, long row_stride, int n_chunks, long chunk_len, long chunk_stride) {
  return rows < 1 || n_chunks < 1 || chunk_len < 1 || row_stride < 0 || chunk_stride < 0 || (n_chunks > 1 && chunk_stride < chunk_len);
}

extern "C" long sda_robust_stats_scratch_bytes(long rows) {
  return rows < 1 ? 0 : rows * (long)(RS_TARGETS * RS_BINS + RS_STATE) * 4;
}

extern "C" int sda_robust_stats(const float* x, long rows, long row_stride, int n_chunks, long chunk_len, long chunk_stride,
                                float* centre, float* scale, void* scratch, long scratch_bytes, void* stream) {
  if (!x || !centre || !scale || !scratch || bad_rows(rows, row_stride, n_chunks, chunk_len, chunk_stride)) { set_error("robust_stats: bad arguments"); return -1; }
  const long N = (long)n_chunks * chunk_len;
  if (N < 2 || N >= (1L << 31)) { set_error("robust_stats: a row of %ld samples (2 .. 2^31 - 1 are served)", N); return -1; }
  if (rows > 65535) { set_error("robust_stats: %ld rows (at most 65535 per call)", rows); return -1; }
  if (scratch_bytes < sda_robust_stats_scratch_bytes(rows)) { set_error("robust_stats: scratch of %ld bytes, %ld needed", scratch_bytes, sda_robust_stats_scratch_bytes(rows)); return -1; }
  // positions in double: a float position is off by whole samples long before N = 3.3 M
  RankTable ranks;
  float frac[3];
  const double qs[3] = {0.25, 0.5, 0.75};
  for (int j = 0; j < 3; ++j) {
    const double pos = qs[j] * (double)(N - 1);
    const long i0 = (long)pos;                         // pos >= 0: truncation is floor
    ranks.rank[2 * j] = (unsigned)i0;
    ranks.rank[2 * j + 1] = (unsigned)(i0 + 1 < N ? i0 + 1 : N - 1);
    frac[j] = (float)(pos - (double)i0);
  }
  hipStream_t st = (hipStream_t)stream;
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch);
  uint32_t* state = hist + rows * (long)(RS_TARGETS * RS_BINS);
  // a row is cut over enough workgroups to fill the chip when the rows alone do not (pooled: 60 rows of 13 MB)
  const long want = (8L * launch_cus() + rows - 1) / rows;
  const long most = (N + RS_WG_ELEMS - 1) / RS_WG_ELEMS;
  const long slices = want < 1 ? 1 : (want > most ? most : want);
  const long share = (N + slices - 1) / slices;
  const unsigned nsl = (unsigned)((N + share - 1) / share);
  hipLaunchKernelGGL(robust_init_kernel, dim3((unsigned)rows), dim3(256), 0, st, state, hist, rows, ranks);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(robust_count_kernel, dim3(nsl, (unsigned)rows), dim3(256), 0, st, x, row_stride, n_chunks, chunk_len, chunk_stride,
                       share, state, hist, pass);
    hipLaunchKernelGGL(robust_resolve_kernel, dim3((unsigned)rows), dim3(256), 0, st, state, hist, rows, pass, frac[0], frac[1], frac[2],
                       centre, scale);
  }
  return check_launch("robust_stats");
}

extern "C" int sda_scale_clamp_rows(const float* x, float* y, long rows, long row_stride, int n_chunks, long chunk_len, long chunk_stride,
                                    const float* centre, const float* scale, float clamp_lim, int clamp, void* stream) {
  if (!x || !y || !centre || !scale || bad_rows(rows, row_stride, n_chunks, chunk_len, chunk_stride)) { set_error("scale_clamp_rows: bad arguments"); return -1; }
  const long pieces = (chunk_len + SC_WG_ELEMS - 1) / SC_WG_ELEMS;
  const long grid = rows * n_chunks * pieces;
  if (pieces > 0x7fffffffL || grid > 0x7fffffffL) { set_error("scale_clamp_rows: %ld workgroups exceed one launch", grid); return -1; }
  hipLaunchKernelGGL(scale_clamp_rows_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, y, row_stride, n_chunks, chunk_len,
                     chunk_stride, (int)pieces, centre, scale, clamp_lim, clamp);
  return check_launch("scale_clamp_rows");
}

extern "C" int sda_gather_baseline_windows(const float* const* win_ptr, const long* win_cstride, float* dst, int B, int C, int T,
                                           int baseline_len, void* stream) {
  if (!win_ptr || !win_cstride || !dst || B < 1 || C < 1 || T < 1 || baseline_len < 0 || baseline_len > T) { set_error("gather_baseline_windows: bad arguments"); return -1; }
  const long rows = (long)B * C;
  const long grid = (rows + 3) / 4;
  if (grid > 0x7fffffffL) { set_error("gather_baseline_windows: %ld rows exceed one launch", rows); return -1; }
  hipLaunchKernelGGL(gather_baseline_windows_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, win_ptr, win_cstride, dst, rows, C, T,
                     baseline_len);
  return check_launch("gather_baseline_windows");
}
