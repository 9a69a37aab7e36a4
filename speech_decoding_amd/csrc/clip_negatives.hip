// clip_negatives — extra speech negatives for the CLIP loss, read IN PLACE from a resident table of plain rows
// (retrieval.WindowBank): negative n is the K = T * row_elems elements from table row starts[n] on.  A negative has no brain
// partner: it enters the brain -> speech soft-max (the column direction of the logits block) only, gets no gradient and no row
// term.  With m_nj = cos(W_n, Z_j) exp(temp):
//     col_lse_j <- logaddexp(col_lse_j, lse_n m_nj)                                   sda_clip_neg_stats
//     D_nj = exp(m_nj - col_lse_j),  G^n[n][j] = D_nj wmax / |W_n|,  cscale^n_j = inv_norm exp(temp) / (wmax |Z_j|),
//     rscale_j += inv_norm sum_n D_nj m_nj / |Z_j|^2,  dtemp += inv_norm sum_nj D_nj m_nj       sda_clip_neg_grad
//     dZ_j[k] += out_scale cscale^n_j sum_n G^n[n][j] table[starts[n] row_elems + k]            sda_clip_dz_windows
// The raw scores S_n[j][n] = <Z_j, W_n> come from sda_sim_gemm_windows with the brain rows as its X operand.  The last entry is
// the hot path: loss_gemm.hip's 256 x 256 tiled dZ product with the speech operand's rows gathered through `starts` — nothing
// is materialised, windows that overlap share their bytes in the caches.  Every sum has one writer and a fixed order.
#include <cstdlib>

#include "sd_common.h"
#include "flat_tile.h"
#include "tr_operand.h"

namespace sda {

namespace {

// block per brain column j: the negatives' logits of the column, their lse in clip_cols_kernel's order, merged into col_lse[j]
__global__ __launch_bounds__(256) void clip_neg_stats_kernel(const float* __restrict__ S, long s_pitch, const float* __restrict__ wsq,
                                                             const float* __restrict__ zsq, const float* __restrict__ temp,
                                                             float* __restrict__ mlog, float* __restrict__ col_lse, int Bn, int N) {
  __shared__ float sh[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  const float alpha = expf(temp[0]);
  const float zn = sqrtf(zsq[j]);
  float mx = -INFINITY;
  for (int n = tid; n < N; n += 256) {
    const float m = S[(size_t)j * s_pitch + n] * (alpha / sqrtf(wsq[n])) / zn;      // clip_rows_kernel's expression
    mlog[(size_t)j * N + n] = m;
    mx = max_nan(mx, m);
  }
  mx = block_max(mx, sh);
  float sum = 0.f;
  for (int n = tid; n < N; n += 256) sum += expf(mlog[(size_t)j * N + n] - mx);     // (each thread re-reads its own writes)
  sum = block_sum(sum, sh);
  if (tid == 0) {
    const float a = col_lse[j], b = mx + logf(sum);
    const float M = max_nan(a, b);
    col_lse[j] = M + logf(expf(a - M) + expf(b - M));
  }
}

// block per column j of G^n (g_pitch of them: the padding columns and the rows N ... nrows - 1 are written as zeros)
template <typename E>
__global__ __launch_bounds__(256) void clip_neg_grad_kernel(const float* __restrict__ mlog, const float* __restrict__ col_lse,
                                                            const float* __restrict__ wsq, const float* __restrict__ zsq,
                                                            const float* __restrict__ temp, float inv_norm, E* __restrict__ Gn,
                                                            long g_pitch, int nrows, float* __restrict__ cscale_n,
                                                            float* __restrict__ rscale, float* __restrict__ colpart, int Bn, int N) {
  __shared__ float sh[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  for (int n = N + tid; n < nrows; n += 256) Elem<E>::st(Gn + (size_t)n * g_pitch + j, 0.f);
  if (j >= Bn) {
    for (int n = tid; n < N; n += 256) Elem<E>::st(Gn + (size_t)n * g_pitch + j, 0.f);
    return;
  }
  float wmax2 = 0.f;
  for (int n = tid; n < N; n += 256) wmax2 = max_nan(wmax2, wsq[n]);
  const float wmax = sqrtf(block_max(wmax2, sh));
  const float cl = col_lse[j];
  float dl = 0.f;
  for (int n = tid; n < N; n += 256) {
    const float m = mlog[(size_t)j * N + n];
    const float d = expf(m - cl);
    dl += d * m;
    Elem<E>::st(Gn + (size_t)n * g_pitch + j, d * (wmax / sqrtf(wsq[n])));
  }
  dl = block_sum(dl, sh) * inv_norm;
  if (tid == 0) {
    rscale[j] += dl / zsq[j];                        // behind sda_clip_grad's write on the same stream: one writer per element
    cscale_n[j] = inv_norm * expf(temp[0]) / (wmax * sqrtf(zsq[j]));
    colpart[j] = dl;
  }
}

// scalars[1] += sum_j colpart[j]: clip_scalars_kernel's order (lane-strided fp64 partials, then lane order), one writer
__global__ void clip_neg_dtemp_kernel(const float* __restrict__ colpart, float* __restrict__ scalars, int Bn) {
  __shared__ double pd[64];
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  double dt = 0.0;
  for (int j = threadIdx.x; j < Bn; j += 64) dt += (double)colpart[j];
  pd[threadIdx.x] = dt;
  __syncthreads();
  if (threadIdx.x != 0) return;
  dt = 0.0;
  for (int k = 0; k < 64; ++k) dt += pd[k];
  scalars[1] = (float)((double)scalars[1] + dt);
}

// ---------------------------------------------------------------------------------------------------------------------------
// out[j][k] += out_scale * cscale[j] * sum_{n < N} G[n][j] * table[starts[n] * Fp + k],   j < Bn, k < K
// clip_dz_tiles_kernel (loss_gemm.hip) with three changes: the speech image's row r of K-step s comes from the window of
// negative min(32 s + r, N - 1) — the per-lane DMA offset is formed per K-step from two wave-uniform reads of `starts` (scalar
// loads: they do not count on the vector-memory counter the DMA ring's waits are written against), relative to the scalar
// base table + base_row * Fp + the tile's first column; K need not be whole 256-element tiles (a chunk of the last tile that
// lies past K is fetched from inside the window instead and feeds outputs that are not stored); the epilogue adds to `out`.
constexpr int DW_TILE = 256;
constexpr int DW_RB = DW_TILE * 2;
constexpr int DW_OP = 32 * DW_RB;
constexpr int DW_STAGE = 2 * DW_OP;
constexpr int DW_NS = 4;
constexpr int DW_PATCH = 16 * 64 * 4;
constexpr int DW_LDS = DW_NS * DW_STAGE + 8 * DW_PATCH;   // 163 840 B

template <typename E>
__global__ __launch_bounds__(512, 2) void clip_dz_windows_kernel(const E* __restrict__ G, const long g_pitch, const E* __restrict__ table,
                                                                 const int* __restrict__ starts, const int base_row, const int rel_max,
                                                                 const long Fp, E* __restrict__ out, const long out_pitch,
                                                                 const float* __restrict__ cscale, const float* __restrict__ out_scale,
                                                                 const int N, const int Bn, const long K, const int ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wid & 1, wj = wid >> 1;               // wave tile: k [wk * 128, +128) x j [wj * 64, +64)
  const int lr = lane & 15, lq = lane >> 4;
  const int j0 = blockIdx.y * DW_TILE;
  const int nks = (N + 31) >> 5;                       // K-steps of 32 negatives; rows past N meet zero coefficients

  const int prow = lane >> 5, pchunk = lane & 31;
  int ychunk[2];                                       // swizzled source column (elements) of this lane's chunk, per piece
  uint32_t ycol[2], goff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = (wid + 8 * h) * 2 + prow;
    const int sw = pchunk ^ chunk_xor<E, DW_RB>(r);
    long jc = (long)j0 + sw * 8;
    if (jc + 8 > g_pitch) jc = g_pitch - 8;
    ychunk[h] = sw * 8;
    ycol[h] = 0;
    goff[h] = (uint32_t)(((size_t)r * g_pitch + (size_t)jc) * sizeof(E));
  }
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
  const size_t gstep = (size_t)32 * g_pitch;
  const E* ys = table;
  const E* gs = G;
  // byte offset of this lane's chunk of piece h in K-step `step`: the window of the row's negative, clamped into the span
  auto step_off = [&](int step, int h) -> uint32_t {
    const int r0 = step * 32 + (wid + 8 * h) * 2;      // wave-uniform
    const int s0 = starts[min(r0, N - 1)], s1 = starts[min(r0 + 1, N - 1)];
    const int rel = min(max((prow ? s1 : s0) - base_row, 0), rel_max);
    return (uint32_t)(((long)rel * Fp + (long)ycol[h]) * (long)sizeof(E));
  };
  auto issue = [&](int buf, int q, uint32_t yo) {      // this wave's q-th piece of a K-step into stage `buf`
    const uint32_t dst = lds_base + buf * DW_STAGE + (wid + 8 * (q & 1)) * 1024;
    if (q < 2) lds_dma16_lean<false>(ys, yo, dst);
    else lds_dma16_lean<false>(gs, goff[q & 1], dst + DW_OP);
  };
  auto prologue = [&](int tile) {
    const long k0 = (long)tile * DW_TILE;
    ys = table + k0;
    gs = G;
#pragma unroll
    for (int h = 0; h < 2; ++h) ycol[h] = (uint32_t)(k0 + ychunk[h] < K ? ychunk[h] : (ychunk[h] & 63));
#pragma unroll
    for (int p = 0; p < DW_NS - 1; ++p) {
      if (p < nks) {
        const uint32_t y0 = step_off(p, 0), y1 = step_off(p, 1);
        issue(p, 0, y0); issue(p, 1, y1); issue(p, 2, 0u); issue(p, 3, 0u);
        gs += gstep;
      }
    }
  };
  uint32_t a_off[8], b_off[4];
#pragma unroll
  for (int a = 0; a < 8; ++a) a_off[a] = tr_offset_bf16<DW_RB>(0, wk * 128 + a * 16, lane);
#pragma unroll
  for (int b = 0; b < 4; ++b) b_off[b] = DW_OP + tr_offset_bf16<DW_RB>(0, wj * 64 + b * 16, lane);

  float* patch = reinterpret_cast<float*>(smem + DW_NS * DW_STAGE + wid * DW_PATCH);
  const float os = out_scale ? out_scale[0] : 1.f;
  const int jr = lane >> 3, kc = (lane & 7) * 8;

  int tile = blockIdx.x;
  if (tile < ntiles) prologue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    f32x4 acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    int cur = 0;
    for (int s = 0; s < nks; ++s) {
      const bool more = s + (DW_NS - 1) < nks;
      uint32_t yo[2] = {0u, 0u};
      if (more) { yo[0] = step_off(s + DW_NS - 1, 0); yo[1] = step_off(s + DW_NS - 1, 1); }
      const int younger = nks - 1 - s;
      if (younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const int nxt = cur == 0 ? DW_NS - 1 : cur - 1;
      const unsigned char* img = smem + cur * DW_STAGE;
      uint4 bf[4], af[8];
#pragma unroll
      for (int b = 0; b < 4; ++b) bf[b] = tr_read_bf16<DW_RB>(img + b_off[b]);
#pragma unroll
      for (int a = 0; a < 8; ++a) af[a] = tr_read_bf16<DW_RB>(img + a_off[a]);
#pragma unroll
      for (int a = 0; a < 8; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = mma16<E>(af[a], bf[b], acc[a][b]);
        if ((a & 1) && more) issue(nxt, a >> 1, yo[(a >> 1) & 1]);
      }
      if (more) gs += gstep;
      cur = cur == DW_NS - 1 ? 0 : cur + 1;
    }
    __syncthreads();                                    // every wave has read its last fragments: the ring is free
    const int next = tile + (int)gridDim.x;
    if (next < ntiles) prologue(next);                  // lands while the epilogue below runs
    // ---- epilogue (clip_dz_tiles_kernel's): acc[a][b]: k = wk * 128 + a * 16 + 4 * lq + r, j = wj * 64 + b * 16 + lr
    const long kbase = (long)tile * DW_TILE + wk * 128;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int a4 = 0; a4 < 4; ++a4) {
          const int ch = (a4 * 4 + lq) ^ lr;
          *reinterpret_cast<f32x4*>(patch + lr * 64 + ch * 4) = acc[half * 4 + a4][b];
        }
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int row = jr + 8 * pass;
          const int j = j0 + wj * 64 + b * 16 + row;
          const f32x4 lo = *reinterpret_cast<const f32x4*>(patch + row * 64 + (((kc >> 2)) ^ row) * 4);
          const f32x4 hi = *reinterpret_cast<const f32x4*>(patch + row * 64 + (((kc >> 2) + 1) ^ row) * 4);
          if (j < Bn && kbase + half * 64 < K) {        // (K is whole 64-element groups: a group is inside or outside)
            const size_t off = (size_t)j * out_pitch + kbase + half * 64 + kc;
            const float cs = cscale[j];
            float o[8], v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            Vec16<E>::load(out + off, o);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = o[e] + os * (cs * v[e]);
            Vec16<E>::store(out + off, v);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the next tile's first K-steps (and this epilogue's own traffic)
  }
}

template <typename E>
int launch_dz_windows(const void* G, long g_pitch, const void* table, const int32_t* starts, int base_row, long Fp, void* out,
                      long out_pitch, const float* cscale, const float* out_scale, int N, int Bn, long K, hipStream_t st) {
  static unsigned long long attr_done = 0;        // per device
  auto kern = clip_dz_windows_kernel<E>;
  if (const int rc = reserve_lds_once(attr_done, kern, DW_LDS, "clip_dz_windows")) return rc;
  const int ntiles = (int)((K + DW_TILE - 1) / DW_TILE);
  const int jblocks = (Bn + DW_TILE - 1) / DW_TILE;
  int gx = launch_cus() / jblocks;                     // one persistent workgroup per CU in all
  if (gx < 1) gx = 1;
  if (gx > ntiles) gx = ntiles;
  hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)jblocks), dim3(512), DW_LDS, st, (const E*)G, g_pitch,
                     (const E*)table + (size_t)base_row * Fp, reinterpret_cast<const int*>(starts), base_row,
                     (int)sda_clip_dz_windows_span(Fp), Fp, (E*)out + (size_t)SDA_ROW_PAD * Fp, out_pitch, cscale, out_scale, N, Bn, K,
                     ntiles);
  return check_launch("clip_dz_windows");
}

}  // namespace
}  // namespace sda

using namespace sda;

extern "C" int sda_clip_neg_stats(const float* S, long s_pitch, const float* wsq, const float* zsq, const float* temp, float* mlog,
                                  float* col_lse, int Bn, int N, void* stream) {
  if (!S || !wsq || !zsq || !temp || !mlog || !col_lse) { set_error("clip_neg_stats: null argument"); return -1; }
  if (Bn < 1 || N < 1 || s_pitch < N) { set_error("clip_neg_stats: need Bn, N >= 1 and s_pitch >= N"); return -1; }
  hipLaunchKernelGGL(clip_neg_stats_kernel, dim3(Bn), dim3(256), 0, (hipStream_t)stream, S, s_pitch, wsq, zsq, temp, mlog, col_lse, Bn, N);
  return check_launch("clip_neg_stats");
}

extern "C" int sda_clip_neg_rows(int N) { return N < 1 ? 0 : (N + 31) / 32 * 32; }

extern "C" int sda_clip_neg_grad(const float* mlog, const float* col_lse, const float* wsq, const float* zsq, const float* temp,
                                 float inv_norm, void* Gn, long g_pitch, float* cscale_n, float* rscale, float* colpart,
                                 float* scalars, int Bn, int N, int dtype, void* stream) {
  if (!mlog || !col_lse || !wsq || !zsq || !temp || !Gn || !cscale_n || !rscale || !colpart || !scalars) {
    set_error("clip_neg_grad: null argument"); return -1;
  }
  if (Bn < 1 || N < 1 || g_pitch < Bn) { set_error("clip_neg_grad: need Bn, N >= 1 and g_pitch >= Bn"); return -1; }
  if (dtype != SDA_BF16 && dtype != SDA_F16) { set_error("clip_neg_grad: 16-bit storage only (there is no fp32 window path)"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const int nrows = sda_clip_neg_rows(N);
  if (dtype == SDA_BF16)
    hipLaunchKernelGGL(clip_neg_grad_kernel<uint16_t>, dim3((unsigned)g_pitch), dim3(256), 0, st, mlog, col_lse, wsq, zsq, temp, inv_norm,
                       (uint16_t*)Gn, g_pitch, nrows, cscale_n, rscale, colpart, Bn, N);
  else
    hipLaunchKernelGGL(clip_neg_grad_kernel<half_t>, dim3((unsigned)g_pitch), dim3(256), 0, st, mlog, col_lse, wsq, zsq, temp, inv_norm,
                       (half_t*)Gn, g_pitch, nrows, cscale_n, rscale, colpart, Bn, N);
  hipLaunchKernelGGL(clip_neg_dtemp_kernel, dim3(1), dim3(64), 0, st, colpart, scalars, Bn);
  return check_launch("clip_neg_grad");
}

extern "C" long sda_clip_dz_windows_span(long row_elems) {
  // the largest starts[n] - base_row one launch serves: its byte offset plus a swizzled 16-byte chunk of the first 512 bytes
  // fits the 32-bit per-lane offset (0: row_elems is not a positive multiple of 64)
  if (row_elems < 64 || row_elems % 64 != 0) return 0;
  const long lim = ((1L << 32) / 2 - 256) / row_elems;
  return lim > 0x7FFFFFFFL ? 0x7FFFFFFFL : lim;
}

extern "C" int sda_clip_dz_windows(const void* Gn, long g_pitch, const void* table, const int32_t* starts, int base_row, long span_rows,
                                   long row_elems, void* out, long out_pitch, const float* cscale_n, const float* out_scale, int N,
                                   int Bn, long K, int dtype, void* stream) {
  if (!Gn || !table || !starts || !out || !cscale_n) { set_error("clip_dz_windows: null argument"); return -1; }
  if (dtype != SDA_BF16 && dtype != SDA_F16) { set_error("clip_dz_windows: 16-bit storage only (there is no fp32 window path)"); return -1; }
  if (row_elems < 64 || row_elems % 64 != 0 || base_row < 0) { set_error("clip_dz_windows: table rows are a positive multiple of 64 elements, base_row >= 0"); return -1; }
  if (N < 1 || Bn < 1 || K < 32 || K % 32 != 0 || K % row_elems != 0) { set_error("clip_dz_windows: N, Bn >= 1 and K a whole number of 64-byte K-steps and of table rows"); return -1; }
  if (g_pitch < Bn || g_pitch < 8 || g_pitch % 8 != 0) { set_error("clip_dz_windows: the coefficient matrix's pitch must cover Bn and be a multiple of 8 elements"); return -1; }
  if (out_pitch < (long)SDA_ROW_PAD * row_elems + K || out_pitch % 8 != 0) { set_error("clip_dz_windows: out_pitch must hold the pad rows and K elements, in 16-byte groups"); return -1; }
  if (span_rows < 0 || span_rows > sda_clip_dz_windows_span(row_elems)) {
    set_error("clip_dz_windows: the windows span %ld table rows, more than the %ld rows (4 GB) one launch addresses", span_rows,
              sda_clip_dz_windows_span(row_elems));
    return -1;
  }
  if ((((uintptr_t)Gn | (uintptr_t)table | (uintptr_t)out) & 15) != 0 || ((uintptr_t)starts & 3) != 0) {
    set_error("clip_dz_windows: Gn, table and out must be 16-byte aligned, starts 4-byte aligned"); return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  return dtype == SDA_BF16
             ? launch_dz_windows<uint16_t>(Gn, g_pitch, table, starts, base_row, row_elems, out, out_pitch, cscale_n, out_scale, N, Bn, K, st)
             : launch_dz_windows<half_t>(Gn, g_pitch, table, starts, base_row, row_elems, out, out_pitch, cscale_n, out_scale, N, Bn, K, st);
}
