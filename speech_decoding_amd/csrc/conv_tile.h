// LDS tile geometry shared by the conv kernels, and the route between them (conv_route.hip).
#pragma once
#include "sd_common.h"

namespace sda {

// One LDS row = one MFMA K-step = 64 bytes (32 bf16 / 16 fp32 input channels).
constexpr int ROW_B = 64;
constexpr int XROWS = TILE_T + 2 * PAD;            // 160: worst-case halo
constexpr int XS_BYTES = XROWS * ROW_B;            // 10 KB

// 64-byte rows, 4 chunks of 16 bytes, chunk' = chunk ^ sw64(row) with sw64 = 2 * bit 2 of the row.
// ds_read_b128 is serviced in four 16-lane groups that are NOT contiguous ({0-3,12-15,20-27}, {4-11,16-19,
// 28-31}, ...): with lane = 16 * chunk + row the MFMA operand read puts rows {0-3,12-15} of one chunk and rows
// {4-11} of the next chunk in one group, and this XOR lands them on 16 distinct 16-byte slots of the 256-byte
// bank row for EVERY starting row (dilated taps start anywhere); measured SQ_LDS_BANK_CONFLICT = 0.
__device__ inline int sw64(int row) { return (row >> 1) & 2; }
__device__ inline int lds_sw64(int row, int chunk) { return row * ROW_B + ((chunk ^ sw64(row)) << 4); }

// Tile geometry of the flat-row-space kernels: written here once, for the kernels and for the route that counts with it.
constexpr int F_UNIT = 128;            // conv3_flat: rows per work unit (one `stats` row each)
constexpr int F_CO = 160;              // conv3_flat: output channels per workgroup
constexpr int G_UNIT = 128;            // conv1_flat: rows per work unit
constexpr int G_CO[2] = {160, 128};    // conv1_flat: output channels per workgroup, in order of preference
constexpr int W_UNIT = 256;            // conv1_wide: rows per tile
constexpr int W_CO[2] = {256, 320};    // conv1_wide: output channels per tile, in order of preference

// conv_route.hip — the ONE place that decides which kernel serves a convolution.  kernel: SDA_CONV_KERNEL_*, or -1 with the
// error set where the flags demand a kernel the shape or storage type cannot have; tile_co: its output-channel tile;
// unit_rows: the rows one [2][Cout_p] row of `stats` covers (TILE: per sample, B * ceil(T / unit_rows) rows; the others: of
// the flat row space, ceil(B * rows_tp(T) / unit_rows) rows).
struct ConvRoute { int kernel, tile_co, unit_rows; };
ConvRoute conv_route(int KS, int Cout_p, int flags, int dtype, bool has_stats);
// Plain row-layout operands, what the flat-row-space kernels address: samples back to back from row SDA_ROW_PAD, one pitch
// for x and w, fully padded weights, `slack_rows` readable rows behind the last sample, 31-bit row and piece offsets.
bool plain_row_layout(const sda_conv_args& a, int slack_rows);

// the routed kernels: what the descriptor must satisfy beyond the route, and the launch
bool conv3_flat_supports(const sda_conv_args& a);
int launch_conv3_flat(const sda_conv_args& a, hipStream_t st);
bool conv1_flat_supports(const sda_conv_args& a);
int launch_conv1_flat(const sda_conv_args& a, hipStream_t st, int tile_co);
bool conv1_wide_supports(const sda_conv_args& a);
int launch_conv1_wide(const sda_conv_args& a, hipStream_t st, int tile_co);

}  // namespace sda
