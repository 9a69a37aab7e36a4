// The pairwise sigmoid loss tail (SigLIP): every (speech i, brain j) pair of a block is its own binary decision,
//   a_ij = S_ij e^temp / (|Y_i| |Z_j|),  l_ij = a_ij + bias,  z_ij = +1 for a positive and -1 for a negative,
//   loss = inv_norm * sum_ij softplus(-z_ij l_ij),  D_ij = d loss / d l_ij / inv_norm = -z_ij sigma(-z_ij l_ij).
// Nothing couples the entries of a row or a column: there is no lse, no cross-rank merge, and a rank's (Bm x Bn) block is
// complete on its own.  With speech labels a pair of two samples that carry the same speech is one more positive
// (SDA_CLIP_DUP_POSITIVE) or takes no part at all (SDA_CLIP_DUP_MASK: no loss term, D = 0 exactly).
// What leaves here feeds the CLIP loss's machinery unchanged: a and diag go to sda_clip_ranks(_labels), (G, rscale, cscale) to
// sda_clip_dz, (Gy, part) to sda_clip_grad_y_finish and sda_clip_dz with the roles exchanged — the layouts, the O(1) scaling of
// G / Gy, the zero row and the zero padding columns are those of sda_clip_grad / sda_clip_grad_y.
// Every sum has an order fixed by the shape (no atomics): two runs give the same bits.
#include "sd_common.h"

namespace sda {

enum { SIG_UNLABELLED = -1 };        // `mode` of the kernels below when there are no labels; else SDA_CLIP_DUP_*

// softplus(x) and sigma(x) from one exponential, t = exp(-|x|) in (0, 1]: no 1 - sigma, nothing overflows.  Past |x| = 104
// t is 0: softplus is x or 0 and sigma is 1 or 0 exactly.
struct SpSig { float sp, sg; };
__device__ inline SpSig softplus_sigmoid(float x) {
  const float t = expf(-fabsf(x));
  const float r = 1.f / (1.f + t);
  SpSig o;
  o.sp = (x > 0.f ? x : 0.f) + log1pf(t);          // (a NaN x: 0 + log1p(NaN) = NaN)
  o.sg = x >= 0.f ? r : t * r;                     // (a NaN x: NaN * NaN)
  return o;
}

// z_ij of one entry: +1, -1, or 0 = the pair is dropped
__device__ inline int pair_sign(int mode, bool pos, bool same) {
  if (pos) return 1;
  if (mode == SIG_UNLABELLED || !same) return -1;
  return mode == SDA_CLIP_DUP_POSITIVE ? 1 : 0;
}

// One workgroup per 64 x 64 tile of the block, lanes along j: wave w takes rows i0 + w, i0 + w + 4, ...; S, a and G move as
// whole 256-byte (128-byte) row segments, and a lane's three column sums need no cross-lane step: the four waves' sums meet in
// LDS and are added in wave order.  The grid covers G's zero row Bm and its padding columns up to g_pitch.
// part[it][j][3] = (sum softplus, sum D a, sum D) over the rows of tile row `it`.
template <typename E>
__global__ __launch_bounds__(256) void sigmoid_pairs_kernel(const float* __restrict__ S, long s_pitch, const float* __restrict__ ysq,
                                                            const float* __restrict__ zsq, const float* __restrict__ temp,
                                                            const float* __restrict__ bias, const int32_t* __restrict__ labels, int mode,
                                                            int col0, float* __restrict__ a_out, float* __restrict__ diag,
                                                            E* __restrict__ G, long g_pitch, float* __restrict__ part, int Bm, int Bn) {
  __shared__ float sh[4];
  __shared__ float acc[4][3][64];
  const int j0 = blockIdx.x * 64, it = blockIdx.y, i0 = it * 64, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = j0 + lane;
  const bool jv = j < Bn, jg = j < g_pitch;
  if (j0 >= Bn) {                                  // a tile of padding columns only: zeros, rows 0 .. Bm
    for (int k = 0; k < 16; ++k) {
      const int i = i0 + w + 4 * k;
      if (i <= Bm && jg) Elem<E>::st(G + (size_t)i * g_pitch + j, 0.f);
    }
    return;
  }
  float ymax2 = 0.f;
  for (int i = tid; i < Bm; i += 256) ymax2 = max_nan(ymax2, ysq[i]);
  const float ymax = sqrtf(block_max(ymax2, sh));
  const float alpha = expf(temp[0]), b = bias[0];
  const float rz = jv ? sqrtf(zsq[j]) : 1.f;
  const int32_t lj = (jv && mode != SIG_UNLABELLED) ? labels[col0 + j] : 0;
  float s_sp = 0.f, s_da = 0.f, s_d = 0.f;
  for (int k = 0; k < 16; ++k) {
    const int i = i0 + w + 4 * k;                  // (uniform over the wave)
    if (i > Bm) break;
    if (i == Bm) {                                 // the zero row behind the contraction
      if (jg) Elem<E>::st(G + (size_t)i * g_pitch + j, 0.f);
      break;
    }
    const float ys = ysq[i];
    const float ri = alpha / sqrtf(ys);
    float g = 0.f;
    if (jv) {
      const float a = S[(size_t)i * s_pitch + j] * ri / rz;
      a_out[(size_t)i * Bn + j] = a;
      const bool pos = i == col0 + j;
      if (pos) diag[i] = a;
      const int z = pair_sign(mode, pos, mode != SIG_UNLABELLED && labels[i] == lj);
      if (z != 0) {                                // (a dropped pair is left out, not multiplied by zero)
        const SpSig v = softplus_sigmoid(z > 0 ? -(a + b) : a + b);
        const float d = z > 0 ? -v.sg : v.sg;
        s_sp += v.sp; s_da += d * a; s_d += d;
        g = d * (ymax / sqrtf(ys));
      }
    }
    if (jg) Elem<E>::st(G + (size_t)i * g_pitch + j, g);
    if (blockIdx.x == 0 && lane == 0 && (i < col0 || i >= col0 + Bn)) diag[i] = 0.f;   // the positive lives in another block
  }
  if (i0 >= Bm) return;                            // (Bm % 64 == 0: the last tile row holds the zero row alone)
  acc[w][0][lane] = s_sp; acc[w][1][lane] = s_da; acc[w][2][lane] = s_d;
  __syncthreads();
  if (tid < 192) {
    const int q = tid >> 6;
    const float s = ((acc[0][q][lane] + acc[1][q][lane]) + acc[2][q][lane]) + acc[3][q][lane];
    if (jv) part[((size_t)it * Bn + j) * 3 + q] = s;
  }
}

// One workgroup: column j's three sums over the tile rows in tile order, rscale / cscale of sda_clip_dz's contract, and the
// block's shares of the loss, d loss / d temp and d loss / d bias — fp64 sums over the columns, thread-strided and then a fixed
// tree over the 256 threads.
__global__ __launch_bounds__(256) void sigmoid_finish_kernel(const float* __restrict__ part, int nparts, const float* __restrict__ ysq,
                                                             const float* __restrict__ zsq, const float* __restrict__ temp,
                                                             float inv_norm, float* __restrict__ rscale, float* __restrict__ cscale,
                                                             float* __restrict__ scalars, int Bm, int Bn) {
  __shared__ float sh[4];
  __shared__ double red[3][256];
  const int tid = threadIdx.x;
  float ymax2 = 0.f;
  for (int i = tid; i < Bm; i += 256) ymax2 = max_nan(ymax2, ysq[i]);
  const float ymax = sqrtf(block_max(ymax2, sh));
  const float alpha = expf(temp[0]);
  double t_sp = 0.0, t_da = 0.0, t_d = 0.0;
  for (int j = tid; j < Bn; j += 256) {
    float sp = 0.f, da = 0.f, d = 0.f;
    for (int p = 0; p < nparts; ++p) {
      const float* q = part + ((size_t)p * Bn + j) * 3;
      sp += q[0]; da += q[1]; d += q[2];
    }
    rscale[j] = da * inv_norm / zsq[j];
    cscale[j] = inv_norm * alpha / (ymax * sqrtf(zsq[j]));
    t_sp += (double)sp; t_da += (double)da; t_d += (double)d;
  }
  red[0][tid] = t_sp; red[1][tid] = t_da; red[2][tid] = t_d;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s]; }
    __syncthreads();
  }
  if (tid < 3) scalars[tid] = (float)(red[tid][0] * (double)inv_norm);
}

// The speech-side twin (clip_grad_y_kernel's shape: one workgroup per (64 columns of Gy, 64 brain rows j), LDS transpose,
// seg / seg_pitch column groups, the zero row Bn): Gy[j][i] = D_ij zmax / |Z_j| with D recomputed from a, bias and the labels
// by the expression of sigmoid_pairs_kernel; part[jt][i] = sum over the workgroup's j of D_ij a_ij (ordered wave sums).
template <typename E>
__global__ __launch_bounds__(256) void sigmoid_grad_y_kernel(const float* __restrict__ a_in, const float* __restrict__ bias,
                                                             const float* __restrict__ zsq, const float* __restrict__ zsq_all, int nz,
                                                             const int32_t* __restrict__ labels, int mode, int col0,
                                                             E* __restrict__ Gy, long gy_pitch, int seg, int seg_pitch,
                                                             float* __restrict__ part, int Bm, int Bn) {
  __shared__ float sh[4];
  __shared__ float tile[64][65];                   // [column of Gy][j]
  const int c0 = blockIdx.x * 64, jt = blockIdx.y, j0 = jt * 64, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nparts = (Bn + 63) / 64;
  float zmax2 = 0.f;
  for (int k = tid; k < nz; k += 256) zmax2 = max_nan(zmax2, zsq_all[k]);
  const float zmax = sqrtf(block_max(zmax2, sh));
  const int j = j0 + lane;
  const bool jv = j < Bn;
  const float b = bias[0];
  const float zf = jv ? zmax / sqrtf(zsq[j]) : 0.f;
  const int32_t lj = (jv && mode != SIG_UNLABELLED) ? labels[col0 + j] : 0;
  for (int k = 0; k < 16; ++k) {
    const int cc = w + 4 * k, c = c0 + cc, s = c / seg_pitch, o = c - s * seg_pitch, i = s * seg + o;
    const bool iv = o < seg && i < Bm;             // (uniform over the wave)
    float g = 0.f, da = 0.f;
    if (iv && jv) {
      const float a = a_in[(size_t)i * Bn + j];
      const int z = pair_sign(mode, i == col0 + j, mode != SIG_UNLABELLED && labels[i] == lj);
      if (z != 0) {
        const SpSig v = softplus_sigmoid(z > 0 ? -(a + b) : a + b);
        const float d = z > 0 ? -v.sg : v.sg;
        g = d * zf;
        da = d * a;
      }
    }
    tile[cc][lane] = g;                            // (selected, never 0 * zf: a non-finite zf stays out of the pad columns)
    da = wave_sum(da);
    if (iv && jt < nparts && lane == 0) part[(size_t)jt * Bm + i] = da;
  }
  __syncthreads();
  for (int k = 0; k < 16; ++k) {
    const int jj = w + 4 * k, jr = j0 + jj;
    if (jr <= Bn) Elem<E>::st(Gy + (size_t)jr * gy_pitch + c0 + lane, jr < Bn ? tile[lane][jj] : 0.f);
  }
}

}  // namespace sda

using namespace sda;

// labels == NULL: the unlabelled loss (mode is ignored); else mode must be one of SDA_CLIP_DUP_*
static int kernel_mode(const int32_t* labels, int mode, bool& bad) {
  bad = labels && mode != SDA_CLIP_DUP_POSITIVE && mode != SDA_CLIP_DUP_MASK;
  return labels ? mode : (int)SIG_UNLABELLED;
}

extern "C" int sda_sigmoid_pairs(const float* S, long s_pitch, const float* ysq, const float* zsq, const float* temp,
                                 const float* bias, const int32_t* labels, int mode, int col0, float* a, float* diag, void* G,
                                 long g_pitch, float* part, int Bm, int Bn, int dtype, void* stream) {
  if (!S || !ysq || !zsq || !temp || !bias || !a || !diag || !G || !part || s_pitch < Bn || g_pitch < Bn) {
    set_error("sigmoid_pairs: null argument, s_pitch < Bn or g_pitch < Bn"); return -1;
  }
  if (Bm < 1 || Bn < 1 || col0 < 0 || (long)col0 + Bn > Bm) { set_error("sigmoid_pairs: need Bm, Bn >= 1 and 0 <= col0, col0 + Bn <= Bm"); return -1; }
  bool bad;
  const int km = kernel_mode(labels, mode, bad);
  if (bad) { set_error("sigmoid_pairs: unknown mode %d", mode); return -1; }
  const dim3 grid((unsigned)((g_pitch + 63) / 64), (unsigned)(Bm / 64 + 1));
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(sigmoid_pairs_kernel<E>, grid, dim3(256), 0, (hipStream_t)stream, S, s_pitch, ysq, zsq, temp, bias,
                                         labels, km, col0, a, diag, (E*)G, g_pitch, part, Bm, Bn));
  return check_launch("sigmoid_pairs");
}

extern "C" int sda_sigmoid_finish(const float* part, int nparts, const float* ysq, const float* zsq, const float* temp,
                                  float inv_norm, float* rscale, float* cscale, float* scalars, int Bm, int Bn, void* stream) {
  if (!part || !ysq || !zsq || !temp || !rscale || !cscale || !scalars || Bm < 1 || Bn < 1 || nparts != (Bm + 63) / 64) {
    set_error("sigmoid_finish: bad arguments (nparts = ceil(Bm / 64))"); return -1;
  }
  hipLaunchKernelGGL(sigmoid_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nparts, ysq, zsq, temp, inv_norm, rscale,
                     cscale, scalars, Bm, Bn);
  return check_launch("sigmoid_finish");
}

extern "C" int sda_sigmoid_grad_y(const float* a, const float* bias, const float* zsq, const float* zsq_all, int nz,
                                  const int32_t* labels, int mode, int col0, void* Gy, long gy_pitch, int seg, int seg_pitch,
                                  float* part, int Bm, int Bn, int dtype, void* stream) {
  if (!a || !bias || !zsq || !zsq_all || !Gy || !part || Bm < 1 || Bn < 1 || nz < Bn || seg < 1 || seg_pitch < seg ||
      seg_pitch % 64 || gy_pitch < seg_pitch || gy_pitch % seg_pitch || (gy_pitch / seg_pitch) * seg < Bm) {
    set_error("sigmoid_grad_y: bad arguments (seg_pitch a multiple of 64, gy_pitch a multiple of seg_pitch covering Bm rows)");
    return -1;
  }
  if (col0 < 0 || (long)col0 + Bn > Bm) { set_error("sigmoid_grad_y: need 0 <= col0, col0 + Bn <= Bm"); return -1; }
  bool bad;
  const int km = kernel_mode(labels, mode, bad);
  if (bad) { set_error("sigmoid_grad_y: unknown mode %d", mode); return -1; }
  const dim3 grid((unsigned)(gy_pitch / 64), (unsigned)(Bn / 64 + 1));
  SDA_DISPATCH(dtype, hipLaunchKernelGGL(sigmoid_grad_y_kernel<E>, grid, dim3(256), 0, (hipStream_t)stream, a, bias, zsq, zsq_all, nz,
                                         labels, km, col0, (E*)Gy, gy_pitch, seg, seg_pitch, part, Bm, Bn));
  return check_launch("sigmoid_grad_y");
}
