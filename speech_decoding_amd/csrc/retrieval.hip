// retrieval — top-k selection over the raw dot products of a block of queries against a candidate bank.
// Reference op this serves: the similarity of models.py:223-232 (Classifier.forward), <q, c> / max(|q| |c|, 1e-8), followed
// by a top-k over candidates that are NOT the batch (the reference only ever ranks a square batch against itself).
//
// One workgroup of 1024 threads owns one query row and walks it ONCE, 4096 columns per step (one 16-byte load per thread, the
// next step's loads in flight behind the current one).  Every column becomes a 64-bit key
//     key = orderable(score) << 32 | (0xFFFFFFFF - column)
// so that "larger key" IS the order of the result: score descending, lower column first on equal scores (clip_ranks_kernel's
// tie rule); keys of one row are distinct and never 0, and 0 pads every list.  The row's current best 64 keys and the
// candidates that beat the 64th of them (`thr`) live in one LDS buffer of 8192 keys.  Step 0 stores its keys straight into the
// buffer and sorts it (bitonic, descending), which sets `thr`; from then on only keys above `thr` are appended — on unordered
// data about 64 ln(M / 4096) of them in the whole rest of the row — and the buffer is sorted again only before it could
// overflow (more than 4096 entries: a row that keeps improving, e.g. ascending scores) and once at the end.  The rank of the
// true candidate is a plain count of the keys above its own, taken in the same pass from the same matrix (integer sums: the
// result does not depend on the order the LDS atomics land in).  Nothing is written but the k results and the rank.
//
// The matrix arrives CHUNK-MAJOR: the columns come in chunks of `chunk_cols` (a multiple of 64), chunk c being a dense
// [n][pad64(columns of the chunk)] fp32 matrix at float offset c * n * chunk_cols — what one similarity GEMM per bank chunk
// leaves behind.  chunk_cols >= M is the plain [n][pad64(M)] matrix.  Padding columns are never read as scores.
#include "sd_common.h"

namespace sda {

namespace {

constexpr int RS_THREADS = 1024;
constexpr int RS_TILE = 4 * RS_THREADS;            // columns per step
constexpr int RS_CAP = 2 * RS_TILE;                // keys the LDS buffer holds (64 KB)
constexpr int RS_KEEP = 64;                        // the list kept between sorts = the largest k served
constexpr int RS_LDS = RS_CAP * 8 + 16;            // + count and rank words

typedef unsigned long long u64;

// fp32 cosine with the reference's clamp.  sqrtf and the division are IEEE-rounded under hipcc's defaults and nothing here can
// contract into an FMA, so the score is the value numpy / torch compute on the CPU from the same three numbers.
__device__ __forceinline__ float cosine(float dot, float qn, float csq) {
  const float s = dot / fmaxf(qn * sqrtf(csq), 1e-8f);
  return s == 0.f ? 0.f : s;                       // -0 and +0 are one score
}
__device__ __forceinline__ u64 make_key(float s, int j) {
  uint32_t b = __float_as_uint(s);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)b << 32) | (u64)(0xFFFFFFFFu - (uint32_t)j);
}
__device__ __forceinline__ float key_score(u64 key) {
  const uint32_t b = (uint32_t)(key >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b);
}

// &S[i][j] (j < M) of the chunk-major matrix: chunk j / chunk_cols, whose pitch is chunk_cols or, for the last one, pad64 of
// what is left.  The one place that knows the layout: the selection and the class reduction both read through it.
__device__ __forceinline__ const float* score_ptr(const float* S, int n, int M, int chunk_cols, int i, int j) {
  const int c = j / chunk_cols, jc = j - c * chunk_cols, rem = M - c * chunk_cols;
  const int pitch = rem >= chunk_cols ? chunk_cols : (rem + 63) / 64 * 64;
  return S + (size_t)c * n * chunk_cols + (size_t)i * pitch + jc;
}

// descending bitonic sort of buf[0, n), n a power of two <= RS_CAP; every thread of the workgroup calls it
__device__ inline void sort_desc(u64* buf, int n, int tid) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (n >> 1); t += RS_THREADS) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const u64 a = buf[lo], b = buf[hi];
        if ((lo & size) == 0 ? a < b : a > b) { buf[lo] = b; buf[hi] = a; }
      }
    }
  }
  __syncthreads();
}

struct Group {                                     // four consecutive columns j .. j + 3 of the row
  f32x4 dot;
  float csq[4];
};

__global__ __launch_bounds__(RS_THREADS) void retrieval_select_kernel(
    const float* __restrict__ S, const float* __restrict__ qsq, const float* __restrict__ csq, const long long* __restrict__ labels,
    long long* __restrict__ indices, float* __restrict__ scores, int32_t* __restrict__ ranks, const int n, const int M, const int k,
    const int chunk_cols) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u64* buf = reinterpret_cast<u64*>(smem);
  int* sh_count = reinterpret_cast<int*>(smem + RS_CAP * 8);
  int* sh_rank = sh_count + 1;
  const int tid = threadIdx.x, i = blockIdx.x;
  const float qn = sqrtf(qsq[i]);

  // columns j .. j + 3 (j % 4 == 0, j < M) of row i; the chunk's pitch is a multiple of 64, so the 16 bytes are in the row
  auto group_ptr = [&](int j) -> const float* { return score_ptr(S, n, M, chunk_cols, i, j); };
  auto load = [&](int j, Group& g) {
    g.dot = f32x4{0.f, 0.f, 0.f, 0.f};
    if (j < M) g.dot = *reinterpret_cast<const f32x4*>(group_ptr(j));
#pragma unroll
    for (int e = 0; e < 4; ++e) g.csq[e] = j + e < M ? csq[j + e] : 0.f;
  };

  // the true candidate's key, from the same matrix as every other score; a label outside the bank leaves rank -1
  u64 lkey = ~0ull;
  bool labelled = false;
  if (labels) {
    const long long lab = labels[i];
    if (lab >= 0 && lab < M) {
      const int j = (int)lab;
      lkey = make_key(cosine(group_ptr(j & ~3)[j & 3], qn, csq[j]), j);
      labelled = true;
    }
  }
  if (tid == 0) { *sh_count = 0; *sh_rank = 0; }

  Group cur, nxt;
  load(tid * 4, cur);
  int beats = 0;
  u64 thr = 0;
  for (int base = 0; base < M; base += RS_TILE) {
    const int j = base + tid * 4;
    load(j + RS_TILE, nxt);
    u64 key[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      key[e] = j + e < M ? make_key(cosine(cur.dot[e], qn, cur.csq[e]), j + e) : 0ull;
      beats += key[e] > lkey ? 1 : 0;
    }
    if (base == 0) {
      // step 0: every key (0 past the row's end) straight into the buffer, sorted at once: it sets the threshold
#pragma unroll
      for (int e = 0; e < 4; ++e) buf[tid * 4 + e] = key[e];
      int cnt = RS_KEEP;
      while (cnt < M && cnt < RS_TILE) cnt <<= 1;
      sort_desc(buf, cnt, tid);
      if (tid == 0) *sh_count = RS_KEEP;
      thr = buf[RS_KEEP - 1];
      __syncthreads();
    } else {
      // at most RS_TILE appends per step, and the step starts with at most RS_CAP - RS_TILE entries
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (key[e] > thr) buf[atomicAdd(sh_count, 1)] = key[e];
      __syncthreads();
      const int cnt = *sh_count;
      __syncthreads();                             // everybody has read the count before the next step appends
      if (cnt > RS_CAP - RS_TILE) {
        int p2 = RS_KEEP;
        while (p2 < cnt) p2 <<= 1;
        for (int t = cnt + tid; t < p2; t += RS_THREADS) buf[t] = 0ull;
        sort_desc(buf, p2, tid);
        if (tid == 0) *sh_count = RS_KEEP;
        thr = buf[RS_KEEP - 1];
        __syncthreads();
      }
    }
    cur = nxt;
  }
  const int cnt = *sh_count;
  if (cnt > RS_KEEP) {
    int p2 = RS_KEEP;
    while (p2 < cnt) p2 <<= 1;
    for (int t = cnt + tid; t < p2; t += RS_THREADS) buf[t] = 0ull;
    sort_desc(buf, p2, tid);
  }
  if (labelled && beats) atomicAdd(sh_rank, beats);
  __syncthreads();
  if (tid < k) {
    const u64 key = buf[tid];
    indices[(size_t)i * k + tid] = (long long)(0xFFFFFFFFu - (uint32_t)key);
    scores[(size_t)i * k + tid] = key_score(key);
  }
  if (ranks && tid == 0) ranks[i] = labelled ? *sh_rank : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Class-level decoding: the bank's M candidates fall into C classes (words), given as a CSR index — order[M], the bank rows
// sorted by class, and offsets[C + 1].  With the logit l[i][j] = scale * cosine(i, j), class c of row i gets
//     "sum"   f = m_c + log sum_{j in c} exp(l - m_c),  m_c the class's OWN maximum      (log of its probability mass)
//     "mean"  that minus log n_c,      "max"  m_c,      an empty class -inf
// and the value written is f - LSE_i, LSE_i the log-sum-exp over classes of the "sum" values (= over the row's M logits).
//
// One workgroup of 1024 threads per query row.  Classes are dealt, CR_GROUPS at a time in class order, to groups of CR_LANES
// adjacent lanes (word frequencies are Zipf-like: most classes have a handful of members, a wave per class would idle): lane a
// of the group takes members a, a + CR_LANES, ... in index order, gathering S[i][order[p]] (the first CR_REG of them stay in
// registers, so a class of up to CR_LANES * CR_REG members is gathered once; a longer one is gathered again for the second
// pass), and the group combines its lanes' maxima and partial sums in a fixed xor tree (4, 2, 1).  A class of more than CR_BIG
// members is left to the whole workgroup (its flag is parked in LDS; every CR_DEFER steps the workgroup meets at a barrier and takes
// the parked classes one by one, so the steps in between run without a barrier): thread t takes members t, t + 1024, ..., combined by a xor tree inside each wave
// (32 ... 1) and then wave 0 ... 15 in order.  Which path a class takes and where each member's term enters the sum depend on
// (order, offsets) alone: no atomics, the same bits on every call.  LSE_i goes the workgroup's way over the C "sum" values,
// which are parked in the row's output until it is known; "max" then walks the classes a second time for the maxima alone.
// Measured on the MI355X (tools/bench_class_decode.py: 256 rows x 32768 candidates in 4096 Zipf-sized classes): 172 us for "sum",
// 3 % of one read of the score block at the copy rate — the gathers are 4-byte loads at the end of a dependent chain, and a
// median class of 2 members leaves most of its 8 lanes idle; an LDS image of the row (128 KB at this size) was not tried
// because it bounds M.  The same pooling as a torch scatter chain takes 2.3 ms.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int CR_THREADS = 1024;
constexpr int CR_WAVES = CR_THREADS / 64;
constexpr int CR_LANES = 8;                        // lanes that share one class
constexpr int CR_GROUPS = CR_THREADS / CR_LANES;   // classes in flight per step
constexpr int CR_REG = 4;                          // members per lane kept in registers between the two passes
constexpr int CR_BIG = 256;                        // a class above this many members is reduced by the whole workgroup
constexpr int CR_DEFER = 64;                       // steps whose big classes are parked (flags in LDS) before the workgroup turns to them
enum { CR_SUM = 0, CR_MEAN = 1, CR_MAX = 2 };

__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int off = CR_LANES / 2; off; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = CR_LANES / 2; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// every thread of the workgroup calls these; sh holds CR_WAVES floats
__device__ __forceinline__ float block_max(float v, float* sh, int tid) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  float t = sh[0];
#pragma unroll
  for (int w = 1; w < CR_WAVES; ++w) t = fmaxf(t, sh[w]);
  return t;
}
__device__ __forceinline__ float block_sum(float v, float* sh, int tid) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  float t = sh[0];
#pragma unroll
  for (int w = 1; w < CR_WAVES; ++w) t += sh[w];
  return t;
}

struct ClassRow {                                  // what one workgroup reads of its query row
  const float* S; const float* csq; const int* order; const int* offsets;
  int n, M, C, chunk_cols, i;
  float qn, scale;
  // logit of the row against member p of the index; an index outside the bank is clamped into it (never read past the row)
  __device__ __forceinline__ float logit(int p) const {
    const int j = min(max(order[p], 0), M - 1);
    return __fmul_rn(scale, cosine(*score_ptr(S, n, M, chunk_cols, i, j), qn, csq[j]));   // a product of its own: no FMA with l - m
  }
  __device__ __forceinline__ void span(int c, int& lo, int& hi) const {
    lo = min(max(offsets[c], 0), M);
    hi = min(max(offsets[c + 1], lo), M);
  }
};

// row[c] = the class's "sum" value (MAXONLY: its maximum - lse) for every class c < C; all 1024 threads call it together
template <bool MAXONLY>
__device__ __forceinline__ void reduce_classes(const ClassRow& r, float* __restrict__ row, float lse, float* sh_red, u64* sh_mask,
                                               int tid) {
  const int grp = tid / CR_LANES, lane = tid % CR_LANES;
  for (int base0 = 0; base0 < r.C; base0 += CR_DEFER * CR_GROUPS) {
    // up to CR_DEFER steps without a barrier: the waves drift apart and hide each other's gather latency
    for (int t = 0; t < CR_DEFER && base0 + t * CR_GROUPS < r.C; ++t) {
      const int c = base0 + t * CR_GROUPS + grp;
      int lo = 0, hi = 0;
      if (c < r.C) r.span(c, lo, hi);
      const bool big = hi - lo > CR_BIG;
      if (big) hi = lo;                            // not this group's: see below
      float v[CR_REG], m = -INFINITY;
#pragma unroll
      for (int e = 0; e < CR_REG; ++e) {
        const int p = lo + lane + e * CR_LANES;
        v[e] = p < hi ? r.logit(p) : -INFINITY;
        m = fmaxf(m, v[e]);
      }
      for (int p = lo + lane + CR_REG * CR_LANES; p < hi; p += CR_LANES) m = fmaxf(m, r.logit(p));
      m = group_max(m);
      float f = m;
      if (!MAXONLY) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < CR_REG; ++e)
          if (lo + lane + e * CR_LANES < hi) s += expf(v[e] - m);
        for (int p = lo + lane + CR_REG * CR_LANES; p < hi; p += CR_LANES) s += expf(r.logit(p) - m);
        s = group_sum(s);
        f = hi > lo ? m + logf(s) : -INFINITY;
      }
      if (lane == 0 && c < r.C && !big) row[c] = MAXONLY ? f - lse : f;
      const u64 flags = __ballot(big);             // the step's big classes: the groups' flags, one ballot per wave
      if ((tid & 63) == 0) sh_mask[t * CR_WAVES + (tid >> 6)] = flags;
    }
    __syncthreads();
    // the big classes of these steps, one after the other, by everybody
    for (int t = 0; t < CR_DEFER && base0 + t * CR_GROUPS < r.C; ++t) {
      for (int w = 0; w < CR_WAVES; ++w) {
        u64 mk = sh_mask[t * CR_WAVES + w] & 0x0101010101010101ull;   // lane 0 of each group
        while (mk) {
          const int bit = __ffsll((long long)mk) - 1;
          mk &= mk - 1;
          const int cb = base0 + t * CR_GROUPS + w * (64 / CR_LANES) + bit / CR_LANES;
          int blo, bhi;
          r.span(cb, blo, bhi);
          const float v0 = blo + tid < bhi ? r.logit(blo + tid) : -INFINITY;
          float bm = v0;
          for (int p = blo + tid + CR_THREADS; p < bhi; p += CR_THREADS) bm = fmaxf(bm, r.logit(p));
          bm = block_max(bm, sh_red, tid);
          float bf = bm;
          if (!MAXONLY) {
            float s = blo + tid < bhi ? expf(v0 - bm) : 0.f;
            for (int p = blo + tid + CR_THREADS; p < bhi; p += CR_THREADS) s += expf(r.logit(p) - bm);
            s = block_sum(s, sh_red, tid);
            bf = bm + logf(s);
          }
          if (tid == 0) row[cb] = MAXONLY ? bf - lse : bf;
        }
      }
    }
    __syncthreads();                               // everybody has read the flags before the next steps write their own
  }
}

__global__ __launch_bounds__(CR_THREADS) void retrieval_class_reduce_kernel(
    const float* __restrict__ S, const float* __restrict__ qsq, const float* __restrict__ csq, const int* __restrict__ order,
    const int* __restrict__ offsets, float* __restrict__ out, float* __restrict__ row_lse, const long pitch, const int n, const int M,
    const int C, const int chunk_cols, const float scale, const int mode) {
  __shared__ float sh_red[CR_WAVES];
  __shared__ u64 sh_mask[CR_DEFER * CR_WAVES];
  const int tid = threadIdx.x, i = blockIdx.x;
  const ClassRow r{S, csq, order, offsets, n, M, C, chunk_cols, i, sqrtf(qsq[i]), scale};
  float* row = out + (size_t)i * pitch;
  reduce_classes<false>(r, row, 0.f, sh_red, sh_mask, tid);
  __syncthreads();                                 // the row's "sum" values, written by other threads, are read below
  // LSE over classes: thread t takes classes t, t + 1024, ... in order (at least one class has a member, so F is finite)
  float F = -INFINITY;
  for (int c = tid; c < C; c += CR_THREADS) F = fmaxf(F, row[c]);
  F = block_max(F, sh_red, tid);
  float s = 0.f;
  for (int c = tid; c < C; c += CR_THREADS) s += expf(row[c] - F);
  s = block_sum(s, sh_red, tid);
  const float lse = F + logf(s);
  if (tid == 0) row_lse[i] = lse;
  if (mode == CR_MAX) {
    __syncthreads();                               // the last read of the "sum" values is behind everybody
    reduce_classes<true>(r, row, lse, sh_red, sh_mask, tid);
    return;
  }
  for (int c = tid; c < C; c += CR_THREADS) {      // each thread rewrites the values it has just read itself
    float f = row[c];
    if (mode == CR_MEAN) {
      int lo, hi;
      r.span(c, lo, hi);
      f = hi > lo ? f - logf((float)(hi - lo)) : -INFINITY;
    }
    row[c] = f - lse;
  }
}

// out[g][c] = log mean_{r in group g} exp(V[r][c]): the rows of group g are rows[goff[g] ... goff[g + 1]), taken in that order
// with the column's own maximum; a column that is -inf in every row stays -inf (no -inf - -inf).  Threads run along c.
constexpr int PR_THREADS = 256;
__global__ __launch_bounds__(PR_THREADS) void retrieval_pool_rows_kernel(
    const float* __restrict__ V, const long v_pitch, const int* __restrict__ rows, const int* __restrict__ goff,
    float* __restrict__ out, const long out_pitch, const int N, const int C, const int ctiles) {
  const int g = blockIdx.x / ctiles, c = (blockIdx.x % ctiles) * PR_THREADS + threadIdx.x;
  if (c >= C) return;
  const int lo = min(max(goff[g], 0), N), hi = min(max(goff[g + 1], lo), N);
  float m = -INFINITY;
  for (int p = lo; p < hi; ++p) m = fmaxf(m, V[(size_t)min(max(rows[p], 0), N - 1) * v_pitch + c]);
  float res = -INFINITY;
  if (m > -INFINITY) {
    float s = 0.f;
    for (int p = lo; p < hi; ++p) s += expf(V[(size_t)min(max(rows[p], 0), N - 1) * v_pitch + c] - m);
    res = (m + logf(s)) - logf((float)(hi - lo));
  }
  out[(size_t)g * out_pitch + c] = res;
}

// Squared norm of candidate m of a windowed bank (retrieval.WindowBank): the T per-row sums from table row starts[m] on.  One
// wavefront per candidate, in the fixed order of gather_baseline_windows_kernel (robust_rows.hip): lane l adds rows l, l + 64,
// ... in order, then the butterfly, so a candidate's norm does not depend on its neighbours or on the call.
__global__ __launch_bounds__(256) void window_sumsq_kernel(const float* __restrict__ row_sq, const int* __restrict__ starts,
                                                           float* __restrict__ out, const int M, const int T) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long m = (long)blockIdx.x * 4 + wid;
  if (m >= M) return;
  const float* w = row_sq + max(starts[m], 0);
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += w[t];
  s = wave_sum(s);
  if (lane == 0) out[m] = s;
}

long scores_floats(int n, int M, int chunk_cols) {
  const long full = M / chunk_cols, rem = M - full * chunk_cols;
  return (long)n * (full * chunk_cols + (rem + 63) / 64 * 64);
}

}  // namespace
}  // namespace sda

using namespace sda;

extern "C" long sda_retrieval_scores_floats(int n, int M, int chunk_cols) {
  if (n < 1 || M < 1 || chunk_cols < 64 || chunk_cols % 64 != 0) {
    set_error("retrieval_scores_floats: n, M >= 1 and chunk_cols a positive multiple of 64");
    return -1;
  }
  return scores_floats(n, M, chunk_cols);
}

extern "C" int sda_retrieval_select(const float* S, const float* qsq, const float* csq, const int64_t* labels, int64_t* indices,
                                    float* scores, int32_t* ranks, int n, int M, int k, int chunk_cols, void* stream) {
  if (!S || !qsq || !csq || !indices || !scores) { set_error("retrieval_select: null argument"); return -1; }
  if ((labels == nullptr) != (ranks == nullptr)) { set_error("retrieval_select: labels and ranks come together or not at all"); return -1; }
  if (n < 1 || M < 1 || M > 0x7FFF0000) { set_error("retrieval_select: n >= 1 and 1 <= M <= 0x7FFF0000"); return -1; }
  if (k < 1 || k > RS_KEEP || k > M) { set_error("retrieval_select: k = %d outside 1 ... min(64, M = %d)", k, M); return -1; }
  if (chunk_cols < 64 || chunk_cols % 64 != 0) { set_error("retrieval_select: chunk_cols must be a positive multiple of 64"); return -1; }
  if (((uintptr_t)S & 15) != 0) { set_error("retrieval_select: the score matrix must be 16-byte aligned"); return -1; }
  static unsigned long long attr_done = 0;         // per device
  if (const int rc = reserve_lds_once(attr_done, retrieval_select_kernel, RS_LDS, "retrieval_select")) return rc;
  hipLaunchKernelGGL(retrieval_select_kernel, dim3((unsigned)n), dim3(RS_THREADS), RS_LDS, (hipStream_t)stream, S, qsq, csq,
                     reinterpret_cast<const long long*>(labels), reinterpret_cast<long long*>(indices), scores, ranks, n, M, k,
                     chunk_cols);
  return check_launch("retrieval_select");
}

extern "C" int sda_retrieval_class_reduce(const float* S, const float* qsq, const float* csq, const int32_t* order,
                                          const int32_t* offsets, float* out, float* row_lse, long out_pitch, int n, int M, int C,
                                          int chunk_cols, float scale, int mode, void* stream) {
  if (!S || !qsq || !csq || !order || !offsets || !out || !row_lse) { set_error("retrieval_class_reduce: null argument"); return -1; }
  if (n < 1 || M < 1 || M > 0x7FFF0000 || C < 1) { set_error("retrieval_class_reduce: n, C >= 1 and 1 <= M <= 0x7FFF0000"); return -1; }
  if (chunk_cols < 64 || chunk_cols % 64 != 0) { set_error("retrieval_class_reduce: chunk_cols must be a positive multiple of 64"); return -1; }
  if (((uintptr_t)S & 15) != 0 || (((uintptr_t)out | (uintptr_t)row_lse | (uintptr_t)qsq | (uintptr_t)csq | (uintptr_t)order | (uintptr_t)offsets) & 3) != 0) {
    set_error("retrieval_class_reduce: the score matrix must be 16-byte aligned, every other array 4-byte aligned");
    return -1;
  }
  if (out_pitch < C) { set_error("retrieval_class_reduce: out_pitch = %ld below C = %d", out_pitch, C); return -1; }
  if (!(scale > 0.f) || !(scale <= 3.402823466e38f)) { set_error("retrieval_class_reduce: scale must be positive and finite"); return -1; }
  if (mode != CR_SUM && mode != CR_MEAN && mode != CR_MAX) { set_error("retrieval_class_reduce: mode %d (0 sum, 1 mean, 2 max)", mode); return -1; }
  hipLaunchKernelGGL(retrieval_class_reduce_kernel, dim3((unsigned)n), dim3(CR_THREADS), 0, (hipStream_t)stream, S, qsq, csq,
                     reinterpret_cast<const int*>(order), reinterpret_cast<const int*>(offsets), out, row_lse, out_pitch, n, M, C,
                     chunk_cols, scale, mode);
  return check_launch("retrieval_class_reduce");
}

extern "C" int sda_retrieval_pool_rows(const float* V, long v_pitch, const int32_t* rows, const int32_t* group_offsets, float* out,
                                       long out_pitch, int N, int G, int C, void* stream) {
  if (!V || !rows || !group_offsets || !out) { set_error("retrieval_pool_rows: null argument"); return -1; }
  if (N < 1 || G < 1 || C < 1) { set_error("retrieval_pool_rows: N, G, C >= 1"); return -1; }
  if (v_pitch < C || out_pitch < C) { set_error("retrieval_pool_rows: a pitch below C = %d", C); return -1; }
  if ((((uintptr_t)V | (uintptr_t)rows | (uintptr_t)group_offsets | (uintptr_t)out) & 3) != 0) {
    set_error("retrieval_pool_rows: every array must be 4-byte aligned");
    return -1;
  }
  const long ctiles = ((long)C + PR_THREADS - 1) / PR_THREADS;
  if (ctiles * G > 0x7FFFFFFFl) { set_error("retrieval_pool_rows: G x ceil(C / %d) exceeds the grid", PR_THREADS); return -1; }
  hipLaunchKernelGGL(retrieval_pool_rows_kernel, dim3((unsigned)(ctiles * G)), dim3(PR_THREADS), 0, (hipStream_t)stream, V, v_pitch,
                     reinterpret_cast<const int*>(rows), reinterpret_cast<const int*>(group_offsets), out, out_pitch, N, C, (int)ctiles);
  return check_launch("retrieval_pool_rows");
}

extern "C" int sda_window_sumsq(const float* row_sq, const int32_t* starts, float* out, int M, int T, void* stream) {
  if (!row_sq || !starts || !out) { set_error("window_sumsq: null argument"); return -1; }
  if (M < 1 || T < 1) { set_error("window_sumsq: M, T >= 1"); return -1; }
  if ((((uintptr_t)row_sq | (uintptr_t)starts | (uintptr_t)out) & 3) != 0) { set_error("window_sumsq: every array must be 4-byte aligned"); return -1; }
  hipLaunchKernelGGL(window_sumsq_kernel, dim3((unsigned)(((long)M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, row_sq,
                     reinterpret_cast<const int*>(starts), out, M, T);
  return check_launch("window_sumsq");
}
