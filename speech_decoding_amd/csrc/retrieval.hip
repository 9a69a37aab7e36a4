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
  auto group_ptr = [&](int j) -> const float* {
    const int c = j / chunk_cols, jc = j - c * chunk_cols, rem = M - c * chunk_cols;
    const int pitch = rem >= chunk_cols ? chunk_cols : (rem + 63) / 64 * 64;
    return S + (size_t)c * n * chunk_cols + (size_t)i * pitch + jc;
  };
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
  if (first_use_on_device(attr_done)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(retrieval_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            RS_LDS) != hipSuccess) {
      set_error("retrieval_select: cannot reserve %d bytes of LDS", RS_LDS);
      return -3;
    }
  }
  hipLaunchKernelGGL(retrieval_select_kernel, dim3((unsigned)n), dim3(RS_THREADS), RS_LDS, (hipStream_t)stream, S, qsq, csq,
                     reinterpret_cast<const long long*>(labels), reinterpret_cast<long long*>(indices), scores, ranks, n, M, k,
                     chunk_cols);
  return check_launch("retrieval_select");
}
