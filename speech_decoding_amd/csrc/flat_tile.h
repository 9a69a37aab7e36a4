// Helpers shared by the flat-tile conv kernels (conv3_flat.hip, conv1_flat.hip).
#pragma once
#include "conv_tile.h"

#include <type_traits>
#include <utility>

namespace sda {

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E)
template <int B, int E, typename F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

template <int N> __device__ __forceinline__ void wait_vmcnt_lit() {
  static_assert(N >= 0 && N <= 8, "add the literal");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
}

// One LDS-DMA piece, lean form: wave-uniform 64-bit source base (an SGPR pair the caller computed with scalar arithmetic
// well ahead — no VALU-written SGPR feeds the load, so no s_nop 4), ONE per-lane byte offset register, and M0 written in
// the statement that reads it (nothing else in these kernels keeps a value in M0, so it is not saved).
// PADDED = true opens with s_nop 4: for the places (a tile's prologue) where hipcc may hand the statement a scalar it has
// just reloaded from a spill lane (v_readlane: a VALU write).  tools/check_dma_hazard.py walks the listing for unpadded ones.
template <bool PADDED = false>
__device__ __forceinline__ void lds_dma16_lean(const void* sbase, uint32_t voff, uint32_t lds_dst) {
  if constexpr (PADDED)
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
  else
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

using TrueC = std::integral_constant<bool, true>;
using FalseC = std::integral_constant<bool, false>;

// The grid of the flat kernels: ONE round of persistent workgroups, each owning a run of `units_per_wg` consecutive
// `unit_rows`-row units of one `tile_co`-channel tile.
struct FlatPlan { int n_units, units_per_wg, runs_per_co, grid; };
inline FlatPlan flat_plan(const sda_conv_args& a, int unit_rows, int tile_co) {
  FlatPlan p;
  const long total_rows = (long)a.B * rows_tp(a.T);
  p.n_units = (int)((total_rows + unit_rows - 1) / unit_rows);
  const int n_co = a.Cout_p / tile_co;
  // two workgroups per CU; one with SDA_CONV_ONE_PER_CU (the caller wants the other half of every CU's LDS for a kernel on
  // another stream: in backward the weight-gradient GEMMs run beside the data-gradient convs)
  const long slots = ((a.flags & SDA_CONV_ONE_PER_CU) ? 1L : 2L) * launch_cus();
  p.units_per_wg = (int)(((long)p.n_units * n_co + slots - 1) / slots);
  if (p.units_per_wg < 1) p.units_per_wg = 1;
  p.runs_per_co = (p.n_units + p.units_per_wg - 1) / p.units_per_wg;
  p.grid = p.runs_per_co * n_co;
  return p;
}

// This workgroup's (channel tile, run) under that plan, in XCD-aware order (blocks i and i + 8 share an XCD/L2): the n_co
// workgroups that read the same input rows are dealt to the same XCD.  Pure speed: any placement is correct.
// (gridDim.x stays unsigned in the division: with an int the compiler emits a signed division and a different kernel)
__device__ __forceinline__ void xcd_block_order(const int n_co, int& co_tile, int& run) {
  const int bid = blockIdx.x;
  const int group = 8 * n_co, full = (int)(gridDim.x / group) * group;
  if (bid < full) {
    const int base = bid / group * group, rem = bid - base;
    co_tile = rem / 8;
    run = base / n_co + (rem & 7);
  } else {
    const int rem = bid - full;
    co_tile = rem % n_co;
    run = full / n_co + rem / n_co;
  }
}

}  // namespace sda
