// The CLIP loss tail with speech labels: two samples of the global batch that carry the same speech segment (lab_i == lab_j)
// are a true match, not a negative.  Every kernel here is the sibling of one in sa_loss.hip — the same block-per-row or
// block-per-column shape, the same ordered block sums, the same G / Gy scaling and layouts — and differs in the coefficient
// D_ij only.  With same_ij = [lab_i == lab_j] and n_i = sum_j same_ij over the GLOBAL batch (sda_clip_label_counts):
//   SDA_CLIP_DUP_POSITIVE  the targets are T_ij = same_ij / n_i:   D_ij = p_row + p_col - 2 T_ij, the soft-max statistics are
//                          the unlabelled ones (sda_clip_logits_stats runs unchanged), a column's loss share is
//                          (row_lse[col0 + j] - pbar_j) + (col_lse_j - pbar_j),  pbar_j = (1 / n_j) sum_i same_{i, col0 + j} l_ij.
//   SDA_CLIP_DUP_MASK      entries with same_ij and i != j leave both soft-max denominators (sda_clip_logits_stats_masked) and
//                          have D_ij = 0; everywhere else D_ij = p'_row + p'_col - 2 delta_ij and the loss terms are the
//                          unlabelled ones.
// Labels are int32 [Bg], one per sample of the global batch: row i has labels[i], local column j has labels[col0 + j].
#include "sd_common.h"

namespace sda {

// block per global sample i: n_i = #{k < Bg : labels[k] == labels[i]} (exact: at most 2^24 samples)
__global__ __launch_bounds__(256) void clip_label_counts_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ counts,
                                                                int Bg) {
  __shared__ float sh[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int32_t li = labels[i];
  float c = 0.f;
  for (int k = tid; k < Bg; k += 256)
    if (labels[k] == li) c += 1.f;
  c = block_sum(c, sh);
  if (tid == 0) counts[i] = (int32_t)(c + 0.5f);
}

// clip_rows_kernel with the repeats of row i's speech (same label, another sample) left out of (max, sum exp); the logits
// themselves are stored unmasked.  A row whose every local column is a repeat has max = -inf and sum = 0 (lse = -inf): the
// cross-rank merge gives such a block no weight.
__global__ __launch_bounds__(256) void clip_rows_masked_kernel(const float* __restrict__ S, long s_pitch, const float* __restrict__ ysq,
                                                               const float* __restrict__ zsq, const float* __restrict__ temp,
                                                               const int32_t* __restrict__ labels, float* __restrict__ logits,
                                                               float* __restrict__ row_max, float* __restrict__ row_sum,
                                                               float* __restrict__ diag, float* __restrict__ row_lse, int Bm, int Bn,
                                                               int col0) {
  __shared__ float sh[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float alpha = expf(temp[0]);
  const float ri = alpha / sqrtf(ysq[i]);
  const int32_t li = labels[i];
  float mx = -INFINITY;
  for (int j = tid; j < Bn; j += 256) {
    const float l = S[(size_t)i * s_pitch + j] * ri / sqrtf(zsq[j]);
    logits[(size_t)i * Bn + j] = l;
    if (col0 + j == i) diag[i] = l;
    if (col0 + j == i || labels[col0 + j] != li) mx = max_nan(mx, l);
  }
  mx = block_max(mx, sh);
  float sum = 0.f;
  for (int j = tid; j < Bn; j += 256)
    if (col0 + j == i || labels[col0 + j] != li) sum += expf(logits[(size_t)i * Bn + j] - mx);
  sum = block_sum(sum, sh);
  if (tid == 0) {
    row_max[i] = mx; row_sum[i] = sum;
    if (row_lse) row_lse[i] = mx + logf(sum);
    if (i < col0 || i >= col0 + Bn) diag[i] = 0.f;
  }
}

// clip_cols_kernel without the repeats of column j's speech (its own positive, row col0 + j, stays)
__global__ __launch_bounds__(256) void clip_cols_masked_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                               float* __restrict__ col_lse, int Bm, int Bn, int col0) {
  __shared__ float sh[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  const int32_t lj = labels[col0 + j];
  float mx = -INFINITY;
  for (int i = tid; i < Bm; i += 256)
    if (i == col0 + j || labels[i] != lj) mx = max_nan(mx, logits[(size_t)i * Bn + j]);
  mx = block_max(mx, sh);
  float sum = 0.f;
  for (int i = tid; i < Bm; i += 256)
    if (i == col0 + j || labels[i] != lj) sum += expf(logits[(size_t)i * Bn + j] - mx);
  sum = block_sum(sum, sh);
  if (tid == 0) col_lse[j] = mx + logf(sum);
}

// D_ij of both modes from one entry's logit, the two lse, whether i and j carry the same speech, whether (i, j) is the
// positive, and 2 / n_j: one expression for clip_grad_labels_kernel and clip_grad_y_labels_kernel (one soft-max for dZ and dY)
template <int MODE>
__device__ inline float label_D(float l, float rl, float cl, bool same, bool pos, float two_over_n) {
  if (MODE == SDA_CLIP_DUP_MASK) {
    if (same && !pos) return 0.f;
    float d = expf(l - rl) + expf(l - cl);
    if (pos) d -= 2.f;
    return d;
  }
  float d = expf(l - rl) + expf(l - cl);
  if (same) d -= two_over_n;
  return d;
}

// clip_grad_kernel with the labelled D: block per local column j; G, rscale, cscale and colpart as there
template <typename E, int MODE>
__global__ __launch_bounds__(256) void clip_grad_labels_kernel(const float* __restrict__ logits, const float* __restrict__ row_lse,
                                                               const float* __restrict__ col_lse, const float* __restrict__ ysq,
                                                               const float* __restrict__ zsq, const float* __restrict__ temp,
                                                               const int32_t* __restrict__ labels, const int32_t* __restrict__ counts,
                                                               float inv_norm, int col0, E* __restrict__ G, long g_pitch,
                                                               float* __restrict__ rscale, float* __restrict__ cscale,
                                                               float* __restrict__ colpart, int Bm, int Bn) {
  __shared__ float sh[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) Elem<E>::st(G + (size_t)Bm * g_pitch + j, 0.f);
  if (j >= Bn) {
    for (int i = tid; i < Bm; i += 256) Elem<E>::st(G + (size_t)i * g_pitch + j, 0.f);
    return;
  }
  float ymax2 = 0.f;
  for (int i = tid; i < Bm; i += 256) ymax2 = max_nan(ymax2, ysq[i]);
  ymax2 = block_max(ymax2, sh);
  const float ymax = sqrtf(ymax2);
  const float alpha = expf(temp[0]);
  const float cl = col_lse[j];
  const int32_t lj = labels[col0 + j];
  const float nj = (float)counts[col0 + j];
  const float two_over_n = 2.f / nj;
  float dl = 0.f, ps = 0.f;
  for (int i = tid; i < Bm; i += 256) {
    const float l = logits[(size_t)i * Bn + j];
    const bool same = labels[i] == lj;
    const float d = label_D<MODE>(l, row_lse[i], cl, same, i == col0 + j, two_over_n);
    // a repeat under MASK is left out, not multiplied by its zero D: a non-finite logit or norm there reaches nothing
    const bool drop = MODE == SDA_CLIP_DUP_MASK && same && i != col0 + j;
    if (!drop) dl += d * l;
    if (MODE == SDA_CLIP_DUP_POSITIVE && same) ps += l;
    Elem<E>::st(G + (size_t)i * g_pitch + j, drop ? 0.f : d * (ymax / sqrtf(ysq[i])));
  }
  dl = block_sum(dl, sh) * inv_norm;
  if (MODE == SDA_CLIP_DUP_POSITIVE) ps = block_sum(ps, sh);
  if (tid == 0) {
    // the mean logit of column j's positives (its own and the repeats), or the one positive's logit
    const float pbar = MODE == SDA_CLIP_DUP_POSITIVE ? ps / nj : logits[(size_t)(col0 + j) * Bn + j];
    rscale[j] = dl / zsq[j];
    cscale[j] = inv_norm * alpha / (ymax * sqrtf(zsq[j]));
    colpart[j * 2 + 0] = (row_lse[col0 + j] - pbar) + (cl - pbar);
    colpart[j * 2 + 1] = dl;
  }
}

// clip_grad_y_kernel with the labelled D: one workgroup per (64 columns of Gy, 64 brain rows j), the same LDS transpose,
// segment layout and partials
template <typename E, int MODE>
__global__ __launch_bounds__(256) void clip_grad_y_labels_kernel(const float* __restrict__ logits, const float* __restrict__ row_lse,
                                                                 const float* __restrict__ col_lse, const float* __restrict__ zsq,
                                                                 const float* __restrict__ zsq_all, int nz,
                                                                 const int32_t* __restrict__ labels, const int32_t* __restrict__ counts,
                                                                 int col0, E* __restrict__ Gy, long gy_pitch, int seg, int seg_pitch,
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
  const float cl = jv ? col_lse[j] : 0.f;
  const float zf = jv ? zmax / sqrtf(zsq[j]) : 0.f;
  const int32_t lj = jv ? labels[col0 + j] : 0;
  const float two_over_n = jv ? 2.f / (float)counts[col0 + j] : 0.f;
  for (int k = 0; k < 16; ++k) {
    const int cc = w + 4 * k, c = c0 + cc, s = c / seg_pitch, o = c - s * seg_pitch, i = s * seg + o;
    const bool iv = o < seg && i < Bm;             // (uniform over the wave)
    float g = 0.f, dl = 0.f;
    if (iv && jv) {
      const float l = logits[(size_t)i * Bn + j];
      const bool same = labels[i] == lj;
      // (a repeat under MASK is left out, not multiplied by its zero D)
      if (!(MODE == SDA_CLIP_DUP_MASK && same && i != col0 + j)) {
        const float d = label_D<MODE>(l, row_lse[i], cl, same, i == col0 + j, two_over_n);
        g = d * zf;
        dl = d * l;
      }
    }
    tile[cc][lane] = g;
    dl = wave_sum(dl);
    if (iv && jt < nparts && lane == 0) part[(size_t)jt * Bm + i] = dl;
  }
  __syncthreads();
  for (int k = 0; k < 16; ++k) {
    const int jj = w + 4 * k, jr = j0 + jj;
    if (jr <= Bn) Elem<E>::st(Gy + (size_t)jr * gy_pitch + c0 + lane, jr < Bn ? tile[lane][jj] : 0.f);
  }
}

// clip_ranks_kernel where a repeat of the row's own speech is never a wrong answer: only columns of another label count
__global__ __launch_bounds__(256) void clip_ranks_labels_kernel(const float* __restrict__ logits, const float* __restrict__ diag,
                                                                const int32_t* __restrict__ labels, int32_t* __restrict__ cnt,
                                                                int Bm, int Bn, int col0) {
  __shared__ float sh[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float d = diag[i];
  const int32_t li = labels[i];
  float c = 0.f;
  for (int j = tid; j < Bn; j += 256) {
    const float l = logits[(size_t)i * Bn + j];
    if (labels[col0 + j] != li && (l > d || (l == d && col0 + j < i))) c += 1.f;
  }
  c = block_sum(c, sh);
  if (tid == 0) cnt[i] = (int32_t)(c + 0.5f);
}

}  // namespace sda

using namespace sda;

static bool bad_mode(int mode) { return mode != SDA_CLIP_DUP_POSITIVE && mode != SDA_CLIP_DUP_MASK; }

extern "C" int sda_clip_label_counts(const int32_t* labels, int32_t* counts, int Bg, void* stream) {
  if (!labels || !counts || Bg < 1 || Bg > (1 << 24)) { set_error("clip_label_counts: bad arguments (1 <= Bg <= 2^24)"); return -1; }
  hipLaunchKernelGGL(clip_label_counts_kernel, dim3(Bg), dim3(256), 0, (hipStream_t)stream, labels, counts, Bg);
  return check_launch("clip_label_counts");
}

extern "C" int sda_clip_logits_stats_masked(const float* S, long s_pitch, const float* ysq, const float* zsq, const float* temp,
                                            const int32_t* labels, float* logits, float* row_max, float* row_sum, float* col_lse,
                                            float* diag, float* row_lse, int Bm, int Bn, int col0, void* stream) {
  if (!S || !ysq || !zsq || !temp || !labels || !logits || !row_max || !row_sum || !col_lse || !diag || Bm < 1 || Bn < 1 ||
      s_pitch < Bn) {
    set_error("clip_logits_stats_masked: bad arguments (Bm, Bn >= 1, s_pitch >= Bn)"); return -1;
  }
  // labels[col0 + j] is read for every local column j
  if (col0 < 0 || (long)col0 + Bn > Bm) { set_error("clip_logits_stats_masked: need 0 <= col0, col0 + Bn <= Bm"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(clip_rows_masked_kernel, dim3(Bm), dim3(256), 0, st, S, s_pitch, ysq, zsq, temp, labels, logits, row_max, row_sum,
                     diag, row_lse, Bm, Bn, col0);
  hipLaunchKernelGGL(clip_cols_masked_kernel, dim3(Bn), dim3(256), 0, st, logits, labels, col_lse, Bm, Bn, col0);
  return check_launch("clip_logits_stats_masked");
}

extern "C" int sda_clip_grad_labels(const float* logits, const float* row_lse, const float* col_lse, const float* ysq,
                                    const float* zsq, const float* temp, const int32_t* labels, const int32_t* counts, int mode,
                                    float inv_norm, int col0, void* G, long g_pitch, float* rscale, float* cscale, float* colpart,
                                    float* scalars, int Bm, int Bn, int dtype, void* stream) {
  if (!logits || !row_lse || !col_lse || !ysq || !zsq || !temp || !labels || !counts || !G || !rscale || !cscale || !colpart ||
      !scalars || g_pitch < Bn) {
    set_error("clip_grad_labels: null argument or g_pitch < Bn"); return -1;
  }
  if (Bm < 1 || Bn < 1 || col0 < 0 || (long)col0 + Bn > Bm) { set_error("clip_grad_labels: need Bm, Bn >= 1 and 0 <= col0, col0 + Bn <= Bm"); return -1; }
  if (bad_mode(mode)) { set_error("clip_grad_labels: unknown mode %d", mode); return -1; }
  hipStream_t st = (hipStream_t)stream;
#define SDA_LAUNCH_GRAD(M)                                                                                                            \
  hipLaunchKernelGGL((clip_grad_labels_kernel<E, M>), dim3((unsigned)g_pitch), dim3(256), 0, st, logits, row_lse, col_lse, ysq, zsq, \
                     temp, labels, counts, inv_norm, col0, (E*)G, g_pitch, rscale, cscale, colpart, Bm, Bn)
  if (mode == SDA_CLIP_DUP_POSITIVE) SDA_DISPATCH(dtype, SDA_LAUNCH_GRAD(SDA_CLIP_DUP_POSITIVE));
  else SDA_DISPATCH(dtype, SDA_LAUNCH_GRAD(SDA_CLIP_DUP_MASK));
#undef SDA_LAUNCH_GRAD
  launch_clip_scalars(colpart, inv_norm, scalars, Bn, st);
  return check_launch("clip_grad_labels");
}

extern "C" int sda_clip_grad_y_labels(const float* logits, const float* row_lse, const float* col_lse, const float* zsq,
                                      const float* zsq_all, int nz, const int32_t* labels, const int32_t* counts, int mode, int col0,
                                      void* Gy, long gy_pitch, int seg, int seg_pitch, float* part, int Bm, int Bn, int dtype,
                                      void* stream) {
  if (!logits || !row_lse || !col_lse || !zsq || !zsq_all || !labels || !counts || !Gy || !part || Bm < 1 || Bn < 1 || nz < Bn ||
      seg < 1 || seg_pitch < seg || seg_pitch % 64 || gy_pitch < seg_pitch || gy_pitch % seg_pitch ||
      (gy_pitch / seg_pitch) * seg < Bm) {
    set_error("clip_grad_y_labels: bad arguments (seg_pitch a multiple of 64, gy_pitch a multiple of seg_pitch covering Bm rows)");
    return -1;
  }
  if (col0 < 0 || (long)col0 + Bn > Bm) { set_error("clip_grad_y_labels: need 0 <= col0, col0 + Bn <= Bm"); return -1; }
  if (bad_mode(mode)) { set_error("clip_grad_y_labels: unknown mode %d", mode); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(gy_pitch / 64), (unsigned)(Bn / 64 + 1));
#define SDA_LAUNCH_GRAD_Y(M)                                                                                                         \
  hipLaunchKernelGGL((clip_grad_y_labels_kernel<E, M>), grid, dim3(256), 0, st, logits, row_lse, col_lse, zsq, zsq_all, nz, labels, \
                     counts, col0, (E*)Gy, gy_pitch, seg, seg_pitch, part, Bm, Bn)
  if (mode == SDA_CLIP_DUP_POSITIVE) SDA_DISPATCH(dtype, SDA_LAUNCH_GRAD_Y(SDA_CLIP_DUP_POSITIVE));
  else SDA_DISPATCH(dtype, SDA_LAUNCH_GRAD_Y(SDA_CLIP_DUP_MASK));
#undef SDA_LAUNCH_GRAD_Y
  return check_launch("clip_grad_y_labels");
}

extern "C" int sda_clip_ranks_labels(const float* logits, const float* diag, const int32_t* labels, int32_t* cnt, int Bm, int Bn,
                                     int col0, void* stream) {
  if (!logits || !diag || !labels || !cnt) { set_error("clip_ranks_labels: null argument"); return -1; }
  if (Bm < 1 || Bn < 1 || col0 < 0 || (long)col0 + Bn > Bm) { set_error("clip_ranks_labels: need Bm, Bn >= 1 and 0 <= col0, col0 + Bn <= Bm"); return -1; }
  hipLaunchKernelGGL(clip_ranks_labels_kernel, dim3(Bm), dim3(256), 0, (hipStream_t)stream, logits, diag, labels, cnt, Bm, Bn, col0);
  return check_launch("clip_ranks_labels");
}
