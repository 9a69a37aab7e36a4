// conv_route — which of sda_conv_gemm's four kernels serves a convolution, decided ONCE: dispatch_conv (conv_gemm.hip) launches
// what conv_route returns, and the public queries below (sda_conv_kernel, sda_conv_tile_co, sda_conv_stats_rows) answer from
// it, so the `stats` rows a caller sizes are the rows the launch writes.  Host only: no kernel lives here.
//
//   flags (of the tiling / epilogue bits)      KS  Cout_p                kernel   tile_co     stats rows
//   EPI_GELU_BWD or EPI_ROW_SUMSQ              3                         refused
//   FLAT_TILES [+ EPI_GLU]                     3   % 160                 FLAT3    160         ceil(B * (T + 16) / 128)
//   EPI_GLU                                    anything else             refused
//   WIDE_TILES [+ GELU_BWD]                    1   % 256 | % 320, 16-bit WIDE     256 | 320   ceil(B * (T + 16) / 256)
//   WIDE_TILES + ROW_SUMSQ                     1   % 256, 16-bit         WIDE     256         (per row)
//   WIDE_TILES                                 1   anything else         refused
//   FLAT_TILES [+ GELU_BWD]                    1   % 160 | % 128         FLAT1    160 | 128   ceil(B * (T + 16) / 128)
//   FLAT_TILES + ROW_SUMSQ                     1   % 128                 FLAT1    128         (per row)
//   ROW_SUMSQ                                  anything else             refused
//   everything else                                                      TILE     sda_conv_tile_co   B * ceil(T / 128)
// The first matching line holds.
#include "conv_tile.h"

namespace sda {

// the tile-per-workgroup kernels' output-channel tile
static int tile_kernel_co(int Cout_p, int KS, bool has_stats) {
  // 1x1 convs whose width divides both ways (640): 128-channel tiles (conv_final1 forward 125 -> 113 us, conv_final2's data
  // gradient 225 -> 195 us; the k = 3 convs and the statistics-row contract stay on 160)
  if (KS == 1 && Cout_p % 128 == 0 && !has_stats) return 128;
  return Cout_p % 160 == 0 ? 160 : Cout_p % 128 == 0 ? 128 : 64;
}

// the first of a kernel's two channel tiles that divides Cout_p (`only`: that one or none), else 0
static int pick_co(const int (&co)[2], int Cout_p, int only = 0) {
  for (const int c : co) if (Cout_p % c == 0 && (!only || c == only)) return c;
  return 0;
}

ConvRoute conv_route(int KS, int Cout_p, int flags, int dtype, bool has_stats) {
  const bool flat = flags & SDA_CONV_FLAT_TILES, wide = flags & SDA_CONV_WIDE_TILES;
  const bool gb = flags & SDA_EPI_GELU_BWD, rsq = flags & SDA_EPI_ROW_SUMSQ;
  const ConvRoute refused = {-1, 0, 0};
  if ((gb || rsq) && KS != 1) { set_error("conv_gemm: SDA_EPI_GELU_BWD and SDA_EPI_ROW_SUMSQ are built for kernel size 1"); return refused; }
  if (flat && KS == 3 && Cout_p % F_CO == 0) return {SDA_CONV_KERNEL_FLAT3, F_CO, F_UNIT};
  if (flags & SDA_EPI_GLU) { set_error("conv_gemm: SDA_EPI_GLU needs SDA_CONV_FLAT_TILES, kernel size 3 and Cout_p %% %d == 0", F_CO); return refused; }
  if (wide && KS == 1) {
    // (an error, not a fallback: this flag names its kernel)
    const int co = dtype == SDA_F32 ? 0 : pick_co(W_CO, Cout_p, rsq ? W_CO[0] : 0);     // (the row sums are per wave: 128 channels of a 256-channel tile)
    if (!co) {
      set_error("conv_gemm: SDA_CONV_WIDE_TILES needs kernel size 1, 16-bit storage and Cout_p %% %d == 0 (or, without SDA_EPI_ROW_SUMSQ, %% %d == 0)",
                W_CO[0], W_CO[1]);
      return refused;
    }
    return {SDA_CONV_KERNEL_WIDE, co, W_UNIT};
  }
  if (flat && KS == 1) {
    const int co = pick_co(G_CO, Cout_p, rsq ? G_CO[1] : 0);                           // (the row sums are per 128-channel tile)
    if (co) return {SDA_CONV_KERNEL_FLAT1, co, G_UNIT};
  }
  if (rsq) {
    set_error("conv_gemm: SDA_EPI_ROW_SUMSQ needs SDA_CONV_FLAT_TILES (or SDA_CONV_WIDE_TILES) and a kernel-1 convolution with Cout_p %% %d == 0", G_CO[1]);
    return refused;
  }
  return {SDA_CONV_KERNEL_TILE, tile_kernel_co(Cout_p, KS, has_stats), TILE_T};
}

bool plain_row_layout(const sda_conv_args& a, int slack_rows) {
  return a.x_row0 == PAD && a.x_pitch == a.w_pitch && a.x_sample_rows == rows_tp(a.T) &&
         a.x_rows_limit >= (long)a.B * rows_tp(a.T) + slack_rows && a.x_rows_limit < (1L << 31) && a.w_rows_limit >= a.Cout_p &&
         (long)a.x_pitch * 16 * (a.dtype == SDA_F32 ? 4 : 2) < (1L << 31);
}

}  // namespace sda

using namespace sda;

extern "C" int sda_conv_kernel(int KS, int Cout_p, int flags, int dtype) {
  if (dtype != SDA_F32 && dtype != SDA_BF16 && dtype != SDA_F16) { set_error("conv_kernel: unknown dtype %d", dtype); return -1; }
  if ((KS != 1 && KS != 3) || Cout_p < 1 || Cout_p % SDA_CH_ALIGN) { set_error("conv_kernel: kernel size %d / Cout_p %d not supported", KS, Cout_p); return -1; }
  return conv_route(KS, Cout_p, flags, dtype, false).kernel;
}

extern "C" int sda_conv_tile_co(int Cout_p, int KS, int has_stats) { return conv_route(KS, Cout_p, 0, SDA_F32, has_stats != 0).tile_co; }

// (no storage type among its arguments: it counts for a type the flags' kernel has; a refused route has no rows, -1)
extern "C" int sda_conv_stats_rows(int B, int T, int KS, int Cout_p, int flags) {
  const ConvRoute r = conv_route(KS, Cout_p, flags, SDA_BF16, true);
  if (r.kernel < 0) return -1;
  if (r.kernel == SDA_CONV_KERNEL_TILE) return B * ((T + r.unit_rows - 1) / r.unit_rows);
  return (int)(((long)B * rows_tp(T) + r.unit_rows - 1) / r.unit_rows);
}
