// The activation row layout's own traffic: (B, C, T) tensors in and out of row-layout buffers, the zero fills that keep
// pad rows and slack zero, and the whole-sample gather.  Every load and store is 16 bytes where the operands allow it.
#include "sd_common.h"

namespace sda {

// ------------------------------------------------------------------------------------------------
// (B, C, T) of storage type S (fp32 / bf16 / fp16)  <->  RL rows of E
// ------------------------------------------------------------------------------------------------
// One pass: a 16-bit input is widened in registers, not through an fp32 copy in HBM.  Widening is exact and the one rounding is
// to E, so every S gives the bits of the fp32 pack of the same values.  A workgroup owns 64 channels x 64 time steps of one
// sample; valid rows get all Cp channels (padding channel `one_ch` ones, -1 = none, the others zero), pad rows are not touched.
template <typename S, typename E>
__global__ __launch_bounds__(256) void pack_rows_kernel(const S* __restrict__ src, E* __restrict__ dst,
                                                        int C, int T, int Cp, int one_ch) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z, c0 = blockIdx.y * 64, t0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int cc = ty; cc < 64; cc += 4) {
    const int c = c0 + cc, t = t0 + tx;
    tile[cc][tx] = (c < C && t < T) ? Elem<S>::ld(src + ((size_t)b * C + c) * T + t) : ((c == one_ch && t < T) ? 1.f : 0.f);
  }
  __syncthreads();
  for (int rr = ty; rr < 64; rr += 4) {
    const int t = t0 + rr;
    if (t < T) Elem<E>::st(dst + ((size_t)b * rows_tp(T) + PAD + t) * Cp + c0 + tx, tile[tx][rr]);
  }
}

// The same for T % (16 / sizeof(S)) == 0 and a 16-byte aligned source: every load and store is 16 bytes.  Loads run along t
// (a channel's 64 steps are 4 lanes x 64 B of bf16 / fp16 or 16 lanes x 16 B of fp32, so a wave reads whole 128 / 256-byte
// runs), stores along c (8 channels of a 16-bit E per lane instead of one: a wave writes 8 rows x 128 B instead of 128 B).
// Same values, same rounding.
template <typename S, typename E>
__global__ __launch_bounds__(256) void pack_rows_vec_kernel(const S* __restrict__ src, E* __restrict__ dst,
                                                            int C, int T, int Cp, int one_ch) {
  __shared__ float tile[64][65];
  constexpr int N = Vec16<S>::N, PER_RUN = 64 / N;          // source elements per load, loads per channel run of the tile
  const int b = blockIdx.z, c0 = blockIdx.y * 64, t0 = blockIdx.x * 64;
#pragma unroll
  for (int k = 0; k < 64 * PER_RUN / 256; ++k) {
    const int idx = threadIdx.x + 256 * k, cc = idx / PER_RUN, tn = (idx % PER_RUN) * N;
    const int c = c0 + cc, t = t0 + tn;
    float v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = 0.f;
    if (t < T) {                                       // (T % N == 0: the N steps are inside or outside together)
      if (c < C) Vec16<S>::load(src + ((size_t)b * C + c) * T + t, v);
      else if (c == one_ch) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = 1.f;
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) tile[cc][tn + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int item = threadIdx.x + 256 * k, chunk = item & 7, rr = item >> 3;
    const int t = t0 + rr;
    if (t < T) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = tile[chunk * 8 + j][rr];
      E* out = dst + ((size_t)b * rows_tp(T) + PAD + t) * Cp + c0 + chunk * 8;
      if constexpr (sizeof(E) == 4) { Vec16<E>::store(out, v); Vec16<E>::store(out + 4, v + 4); }
      else Vec16<E>::store(out, v);
    }
  }
}

template <typename E, typename O>
__global__ __launch_bounds__(256) void unpack_rows_kernel(const E* __restrict__ src, O* __restrict__ dst,
                                                          int C, int T, int Cp) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z, c0 = blockIdx.y * 64, t0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < 64; rr += 4) {
    const int t = t0 + rr;
    tile[rr][tx] = (t < T) ? Elem<E>::ld(src + ((size_t)b * rows_tp(T) + PAD + t) * Cp + c0 + tx) : 0.f;
  }
  __syncthreads();
  for (int cc = ty; cc < 64; cc += 4) {
    const int c = c0 + cc, t = t0 + tx;
    if (c < C && t < T) Elem<O>::st(dst + ((size_t)b * C + c) * T + t, tile[tx][cc]);
  }
}

// rows of a row-layout buffer that no kernel writes but every conv reads as zeros: the PAD rows in front of each sample and
// the slack behind the last one (16-byte stores; a row is Cp * sizeof(E) bytes, a multiple of 128)
__global__ __launch_bounds__(256) void zero_pad_rows_kernel(uint4* __restrict__ buf, int B, int Tp, long rows_alloc, int row_vec) {
  const long pad_vecs = (long)B * PAD * row_vec, tail_vecs = (rows_alloc - (long)B * Tp) * row_vec;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < pad_vecs + tail_vecs; i += (long)gridDim.x * 256) {
    long v;
    if (i < pad_vecs) { const long b = i / ((long)PAD * row_vec), r = i - b * PAD * row_vec; v = b * Tp * row_vec + r; }
    else v = (long)B * Tp * row_vec + (i - pad_vecs);
    buf[v] = make_uint4(0u, 0u, 0u, 0u);
  }
}
// zero `n16` 16-byte vectors + `tail` trailing bytes
__global__ __launch_bounds__(256) void fill_zero_kernel(uint4* __restrict__ p, long n16, int tail) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) reinterpret_cast<unsigned char*>(p + n16)[threadIdx.x] = 0;
}
// dst sample b = table sample idx[b]: whole samples of `vecs` 16-byte vectors (a row-layout sample is (T + PAD) * Cp contiguous
// elements, pad rows included, so a gathered batch IS a row-layout buffer); blockIdx.y = b
__global__ __launch_bounds__(256) void gather_samples_kernel(const uint4* __restrict__ table, const long* __restrict__ idx,
                                                             uint4* __restrict__ dst, long vecs) {
  const uint4* __restrict__ src = table + (size_t)idx[blockIdx.y] * vecs;
  uint4* __restrict__ out = dst + (size_t)blockIdx.y * vecs;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long step = (long)gridDim.x * 256;
  for (; i + 3 * step < vecs; i += 4 * step) {            // four loads in flight per lane
    const uint4 a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
    out[i] = a; out[i + step] = b; out[i + 2 * step] = c; out[i + 3 * step] = d;
  }
  for (; i < vecs; i += step) out[i] = src[i];
}
// dst sample b = the T rows from row starts[idx[b]] on of a table of plain rows (row_vec 16-byte vectors each), behind PAD zero
// rows: a window of a resident track gathered straight into the row layout.  ONE launch writes every vector of dst — pad rows,
// windows and the slack behind the last sample (slack_vecs, shared out over the whole grid) — so dst may arrive uninitialised.
// A candidate outside [0, M) or a start outside [0, table_rows - T] gives a sample of zeros: nothing outside the table is read.
// blockIdx.y = b; a window is T * row_vec contiguous vectors of the table, copied like gather_samples_kernel copies a sample.
__global__ __launch_bounds__(256) void gather_windows_kernel(const uint4* __restrict__ table, long table_rows,
                                                             const int* __restrict__ starts, int M, const long* __restrict__ idx,
                                                             uint4* __restrict__ dst, int T, int row_vec, long slack_vecs) {
  const long pad_vecs = (long)PAD * row_vec, vecs = (long)T * row_vec;
  const long m = idx[blockIdx.y];
  const long s = (m >= 0 && m < M) ? (long)starts[m] : -1;
  const bool inside = s >= 0 && s <= table_rows - T;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  uint4* __restrict__ out = dst + (size_t)blockIdx.y * (pad_vecs + vecs);
  const long first = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  for (long i = first; i < pad_vecs; i += step) out[i] = zero;
  out += pad_vecs;
  long i = first;
  if (inside) {
    const uint4* __restrict__ src = table + (size_t)s * row_vec;
    for (; i + 3 * step < vecs; i += 4 * step) {            // four loads in flight per lane
      const uint4 a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
      out[i] = a; out[i + step] = b; out[i + 2 * step] = c; out[i + 3 * step] = d;
    }
    for (; i < vecs; i += step) out[i] = src[i];
  } else {
    for (; i < vecs; i += step) out[i] = zero;
  }
  uint4* __restrict__ slack = dst + (size_t)gridDim.y * (pad_vecs + vecs);
  for (long j = (long)blockIdx.y * step + first; j < slack_vecs; j += (long)gridDim.y * step) slack[j] = zero;
}
__global__ void scalar_mul_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] * b[0];
}
}  // namespace sda

using namespace sda;

extern "C" int sda_zero_pad_rows(void* buf, int B, int T, int Cp, int dtype, void* stream) {
  if (!buf || B < 1 || T < 1 || Cp % 64) { set_error("zero_pad_rows: bad arguments"); return -1; }
  const int row_vec = Cp * (dtype == SDA_F32 ? 4 : 2) / 16;
  const long n = ((long)B * PAD + (rows_alloc(B, T) - (long)B * rows_tp(T))) * row_vec;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(zero_pad_rows_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream,
                     (uint4*)buf, B, rows_tp(T), rows_alloc(B, T), row_vec);
  return check_launch("zero_pad_rows");
}

extern "C" int sda_fill_zero(void* p, long nbytes, void* stream) {
  if (!p || nbytes < 1 || (reinterpret_cast<uintptr_t>(p) & 15)) { set_error("fill_zero: null, empty or unaligned buffer"); return -1; }
  const long n16 = nbytes / 16;
  const long blocks = (n16 + 255) / 256;
  hipLaunchKernelGGL(fill_zero_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks))), dim3(256), 0, (hipStream_t)stream,
                     (uint4*)p, n16, (int)(nbytes - n16 * 16));
  return check_launch("fill_zero");
}

extern "C" int sda_gather_samples(const void* table, const long* idx, void* dst, int B, long sample_bytes, void* stream) {
  if (!table || !idx || !dst || B < 1 || sample_bytes < 16 || sample_bytes % 16 || (reinterpret_cast<uintptr_t>(table) & 15) ||
      (reinterpret_cast<uintptr_t>(dst) & 15)) {
    set_error("gather_samples: bad arguments (samples are whole 16-byte vectors)"); return -1;
  }
  const long vecs = sample_bytes / 16;
  long bx = (vecs + 256 * 4 - 1) / (256 * 4);
  const long want = (8L * launch_cus() + B - 1) / B;      // ~8 workgroups per CU over the whole batch
  if (bx > want) bx = want;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(gather_samples_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)table, idx, (uint4*)dst, vecs);
  return check_launch("gather_samples");
}

extern "C" int sda_gather_windows(const void* table, long table_rows, const int32_t* starts, int M, const long* idx, void* dst,
                                  int B, int T, long row_bytes, void* stream) {
  if (!table || !starts || !idx || !dst) { set_error("gather_windows: null pointer (table, starts, idx and dst are required)"); return -1; }
  if (B < 1 || T < 1 || M < 1) { set_error("gather_windows: B=%d, T=%d, M=%d must all be at least 1", B, T, M); return -1; }
  if (B > 65535) { set_error("gather_windows: B=%d above 65535 samples per launch", B); return -1; }
  if (table_rows < T) { set_error("gather_windows: a table of %ld rows holds no window of T=%d rows", table_rows, T); return -1; }
  if (row_bytes < 128 || row_bytes % 128 || row_bytes > (1L << 30)) {
    set_error("gather_windows: row_bytes=%ld is not a multiple of 128 up to 2^30 (a row is pad64(F) elements)", row_bytes); return -1;
  }
  if ((reinterpret_cast<uintptr_t>(table) & 15) || (reinterpret_cast<uintptr_t>(dst) & 15)) {
    set_error("gather_windows: table and dst must be 16-byte aligned"); return -1;
  }
  const int row_vec = (int)(row_bytes / 16);
  const long vecs = (long)T * row_vec;
  long bx = (vecs + 256 * 8 - 1) / (256 * 8);             // at least eight vectors of a window per lane
  const long want = (8L * launch_cus() + B - 1) / B;      // ~8 workgroups per CU over the whole batch
  if (bx > want) bx = want;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)table, table_rows, (const int*)starts, M, idx, (uint4*)dst, T, row_vec,
                     (rows_alloc(B, T) - (long)B * rows_tp(T)) * row_vec);
  return check_launch("gather_windows");
}

extern "C" int sda_scalar_mul(const float* a, const float* b, float* out, int n, void* stream) {
  if (!a || !b || !out || n < 1) { set_error("scalar_mul: bad arguments"); return -1; }
  hipLaunchKernelGGL(scalar_mul_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, a, b, out, n);
  return check_launch("scalar_mul");
}

// The one launch of the pack: 16-byte loads where the source allows them, else one element per lane.  one_ch: -1 = none.
template <typename S>
static int launch_pack_rows(const S* src, void* dst, int B, int C, int T, int Cp, int one_ch, int dtype, void* stream,
                            const char* what) {
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((T + 63) / 64, Cp / 64, B);
  if (T % Vec16<S>::N == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    SDA_DISPATCH(dtype, hipLaunchKernelGGL((pack_rows_vec_kernel<S, E>), grid, dim3(256), 0, st, src, (E*)dst, C, T, Cp, one_ch));
  } else {
    SDA_DISPATCH(dtype, hipLaunchKernelGGL((pack_rows_kernel<S, E>), grid, dim3(256), 0, st, src, (E*)dst, C, T, Cp, one_ch));
  }
  return check_launch(what);
}

extern "C" int sda_pack_rows(const float* src, void* dst, int B, int C, int T, int Cp, int dtype, void* stream) {
  if (!src || !dst || Cp % 64 || C > Cp || B < 1) { set_error("pack_rows: bad arguments"); return -1; }
  return launch_pack_rows(src, dst, B, C, T, Cp, -1, dtype, stream, "pack_rows");
}

extern "C" int sda_pack_rows_ones(const float* src, void* dst, int B, int C, int T, int Cp, int ones_channel, int dtype,
                                  void* stream) {
  if (!src || !dst || Cp % 64 || C > Cp || B < 1 || ones_channel < C || ones_channel >= Cp) {
    set_error("pack_rows_ones: bad arguments (the constant channel must be a padding channel)"); return -1;
  }
  return launch_pack_rows(src, dst, B, C, T, Cp, ones_channel, dtype, stream, "pack_rows_ones");
}

// true for memory the current process allocated on a device (or managed memory); false for host memory, or with no device.
// A failed query leaves a runtime error behind, which is cleared here so that the next launch check does not report it.
static bool device_memory(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// any source dtype; off the step's host path, so it can afford the pointer query the two fp32 entry points do without
extern "C" int sda_pack_rows_typed(const void* src, void* dst, int B, int C, int T, int Cp, int src_dtype, int dtype,
                                   void* stream) {
  if (!src || !dst || B < 1 || C < 1 || T < 1 || Cp % 64 || C > Cp || B > 65535) {
    set_error("pack_rows_typed: bad arguments (need 1 <= C <= Cp, Cp a multiple of 64)"); return -1;
  }
  if (src_dtype < SDA_F32 || src_dtype > SDA_F16 || dtype < SDA_F32 || dtype > SDA_F16) {
    set_error("pack_rows_typed: unknown dtype (source %d, destination %d)", src_dtype, dtype); return -1;
  }
  if (!device_memory(src) || !device_memory(dst)) { set_error("pack_rows_typed: src and dst must be device memory"); return -1; }
  if (src_dtype == SDA_F32) return launch_pack_rows((const float*)src, dst, B, C, T, Cp, -1, dtype, stream, "pack_rows_typed");
  if (src_dtype == SDA_BF16) return launch_pack_rows((const uint16_t*)src, dst, B, C, T, Cp, -1, dtype, stream, "pack_rows_typed");
  return launch_pack_rows((const half_t*)src, dst, B, C, T, Cp, -1, dtype, stream, "pack_rows_typed");
}

template <typename O>
static int launch_unpack_rows(const void* src, O* dst, int B, int C, int T, int Cp, int dtype, void* stream) {
  SDA_DISPATCH(dtype, hipLaunchKernelGGL((unpack_rows_kernel<E, O>), dim3((T + 63) / 64, Cp / 64, B), dim3(256), 0, (hipStream_t)stream,
                                         (const E*)src, dst, C, T, Cp));
  return check_launch("unpack_rows");
}

// RL of `dtype` -> a (B, C, T) tensor of dst_dtype: one rounding where the stored value does not fit the output type
extern "C" int sda_unpack_rows_typed(const void* src, void* dst, int B, int C, int T, int Cp, int dtype, int dst_dtype,
                                     void* stream) {
  if (!src || !dst || Cp % 64 || C > Cp || B < 1) { set_error("unpack_rows: bad arguments"); return -1; }
  if (dst_dtype == SDA_F32) return launch_unpack_rows(src, (float*)dst, B, C, T, Cp, dtype, stream);
  if (dst_dtype == SDA_BF16) return launch_unpack_rows(src, (uint16_t*)dst, B, C, T, Cp, dtype, stream);
  if (dst_dtype == SDA_F16) return launch_unpack_rows(src, (half_t*)dst, B, C, T, Cp, dtype, stream);
  set_error("unpack_rows: unknown output dtype %d", dst_dtype);
  return -1;
}

extern "C" int sda_unpack_rows(const void* src, float* dst, int B, int C, int T, int Cp, int dtype, void* stream) {
  return sda_unpack_rows_typed(src, dst, B, C, T, Cp, dtype, SDA_F32, stream);
}
