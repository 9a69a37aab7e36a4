/* sd_amd.h — C ABI of libsdamd.so: MI355X (gfx950) kernels for the contrastive training hot path of
 * SeanNobel/speech-decoding (BrainEncoder + CLIPLoss + Classifier).
 *
 * The reference is pure Python/PyTorch and has no FFI of its own: what a binding
 * would replace are the aten calls made by
 *     speech_decoding/models.py:45-65    SpatialAttention.forward      -> sda_sa_weights_*, sda_conv_gemm
 *     speech_decoding/models.py:111-117  SubjectBlock.forward          -> sda_conv_gemm (widx = subject)
 *     speech_decoding/models.py:152-166  ConvBlock.forward             -> sda_conv_gemm, sda_bn_*, sda_glu_*
 *     speech_decoding/models.py:191-196  BrainEncoder.forward          -> sda_conv_gemm (GELU epilogue)
 *     speech_decoding/utils/loss.py:58-79 CLIPLoss.forward (fast path) -> sda_rows_sumsq, sda_conv_gemm (split-K),
 *                                                                         sda_clip_logits_stats, sda_clip_grad(_y),
 *                                                                         sda_wgrad_gemm (typed output)
 *     speech_decoding/models.py:208-248  Classifier.forward            -> sda_clip_ranks
 * and their autograd backward.  Every entry point takes plain device pointers, sizes and a
 * hipStream_t (passed as void*); no torch types cross this boundary.  All functions return 0 on
 * success and a negative code on failure; sda_last_error() gives the message.
 *
 * Activation "row layout" (RL): a (B, C, T) tensor is stored channels-last as rows of Cp elements,
 *     row(b, t) = b * (T + SDA_ROW_PAD) + SDA_ROW_PAD + t,        Cp = C rounded up to 64,
 * with all padding rows / channels equal to zero, in a buffer of sda_rows_alloc(B, T) rows.
 */
#ifndef SD_AMD_H
#define SD_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDA_ABI_VERSION 4   /* 2: sda_conv_args gained glu_out / glu_gate, sda_pack_desc gained glu_tile, flag 16384 = SDA_CONV_FLAT_TILES;
                               (still 2, should have been bumped: sda_wgrad_args.acc_scale, new arguments of sda_bn_finalize,
                               sda_clip_logits_stats and sda_clip_grad, new entries sda_clip_dz / sda_param_gemm / sda_copy3d)
                               3: sda_wgrad_args.flags (SDA_WGRAD_FLAT_ROWS), sda_stream_create_cumask / sda_stream_create_priority / sda_stream_destroy, sda_sim_gemm / sda_sim_gemm_ksplit,
                               conv3_flat takes x_pitch == w_pitch only
                               4: sda_fill_zero, sda_gather_samples, sda_clip_merge_rows; SDA_WGRAD_FLAT_ROWS with a sample permutation;
                                  sda_clip_dz serves more than 256 speech rows (256 x 256 tiles); SDA_CONV_WIDE_TILES
                                  (still 4, additions only: sda_robust_stats / sda_robust_stats_scratch_bytes, sda_scale_clamp_rows,
                                  sda_gather_baseline_windows — the Brennan2018 input path; sda_window_gemm_f32 — FIR filter / sinc resampler;
                                  sda_mel_power_f32 — power, mel filterbank and log behind the STFT;
                                  sda_stft_fft_f32 — the STFT as a power-of-two FFT;
                                  sda_conv_tile_co / sda_wgrad_tile_m — the output-channel tile rules, asked instead of mirrored;
                                  sda_sim_gemm_windows / sda_sim_gemm_windows_span / sda_window_sumsq — decoding against windows of
                                  continuous speech tracks;
                                  sda_gather_windows — training batches gathered from such tracks;
                                  sda_lagged_cov_f32 / sda_lagged_cov_slices / sda_lagged_cov_scratch_floats — the lag products of the
                                  time-lagged ridge baseline;
                                  sda_conv_kernel — which kernel sda_conv_gemm routes a convolution to, asked instead of mirrored;
                                  sda_clip_label_counts / sda_clip_logits_stats_masked / sda_clip_grad_labels / sda_clip_grad_y_labels /
                                  sda_clip_ranks_labels — the loss tail with speech labels;
                                  sda_sigmoid_pairs / sda_sigmoid_finish / sda_sigmoid_grad_y — the pairwise sigmoid loss tail;
                                  sda_clip_neg_stats / sda_clip_neg_rows / sda_clip_neg_grad / sda_clip_dz_windows /
                                  sda_clip_dz_windows_span — extra speech negatives read in place from resident tracks) */
#define SDA_ROW_PAD 16
#define SDA_CH_ALIGN 64

enum { SDA_F32 = 0, SDA_BF16 = 1, SDA_F16 = 2 };   /* storage + MFMA operand type; accumulation is always fp32 */

/* conv_gemm epilogue flags.  sda_conv_gemm refuses a `flags` word with any bit that is not named here. */
enum { SDA_EPI_GELU = 1,
       SDA_EPI_GLU_BWD = 4,         /* the conv's output is the gradient dy entering an F.glu whose forward kept (out, gate) (SDA_EPI_GLU):
                                       y [rows][2 * Cout_p] = [dy * sig(gate) | dy * out * (1 - sig(gate))] (the GLU backward, written
                                       instead of dy), `stats` rows = per-tile column sums of the two halves ([tile][0] value half,
                                       [tile][1] gate half: the bias gradient of the conv that fed the GLU).  Needs glu_out, glu_gate and
                                       stats; the tile-per-workgroup kernels only (not SDA_CONV_FLAT_TILES); no GELU / bn_x */
       SDA_EPI_GLU = 2,             /* with SDA_CONV_FLAT_TILES: the conv's Cout_p = 2 * Hp channels are [value | gate] pairs
                                       laid out per 160-channel tile as 80 value + 80 gate channels (weights and bias packed with
                                       glu_tile = 80); y [rows][Hp] = value * sigmoid(gate) (models.py:164, F.glu), both as
                                       rounded to the storage type; y_pre [rows][Hp] = gate, or NULL.  No res / stats / bn_x */
       SDA_CONV_SINGLE_TILE = 4096, /* force one 128-row tile per workgroup */
       SDA_CONV_PAIR_TILES = 8192,  /* two tiles per workgroup sharing one weight slab (default: one) */
       SDA_CONV_ONE_PER_CU = 32768, /* with SDA_CONV_FLAT_TILES: at most one workgroup per CU (half the LDS stays free) */
       SDA_CONV_FLAT_TILES = 16384, /* kernel size 3 with Cout_p % 160 == 0: 256-row x 160-channel tiles cut from the
                                       flat row space, two workgroups per CU (conv3_flat.hip); kernel size 1 with
                                       Cout_p % 160 == 0 or Cout_p % 128 == 0: the same tiling (conv1_flat.hip).  Other shapes
                                       ignore the flag (sda_conv_kernel tells), and so does a kernel-size-1 launch that writes no
                                       statistics and is not a plain row-layout convolution with shared weights and no residual;
                                       one that writes statistics (SDA_EPI_GELU_BWD, SDA_EPI_ROW_SUMSQ, `stats`) is refused there,
                                       never served by a kernel with another row count.  `stats` has sda_conv_stats_rows(...)
                                       rows: those of the kernel that runs */
       SDA_CONV_FLAT_STAGGER = 1024,/* with SDA_CONV_FLAT_TILES, kernel size 3 (conv3_flat.hip): the second workgroup of a CU takes its
                                       128-row tile(s) first and its 256-row tiles after them, the first workgroup the other way
                                       round, so that the two reach their epilogues at different times.  Same results either way;
                                       every other kernel ignores the flag */
       SDA_CONV_WIDE_TILES = 524288,/* kernel size 1, 16-bit storage, Cout_p % 256 == 0 or % 320 == 0, shared weights, no residual: 256-row x
                                       256- / 320-channel tiles of the flat row space, eight waves, one persistent workgroup per CU
                                       (conv1_wide.hip); takes SDA_EPI_GELU (+ y_pre), SDA_EPI_GELU_BWD (`stats` = one row per 256-row
                                       tile: sda_conv_stats_rows), SDA_EPI_ROW_SUMSQ (Cout_p % 256 == 0).  Any other shape with this
                                       flag is an error, not a fallback */
       SDA_CONV_WAVE_PRIO = 1048576,/* the tile-per-workgroup kernels: the launch's waves run at s_setprio 3 (they win a SIMD's issue
                                       arbitration against co-resident waves of other kernels) */
       SDA_EPI_GELU_BWD = 65536,    /* kernel size 1 (any of its kernels): the conv's output is the gradient entering a GELU whose input u = bn_x ([rows][Cout_p],
                                       same layout as y) the forward kept: y = round(conv) * GELU'(u) (what sda_gelu_backward_colsum
                                       computes from the stored gradient), `stats` rows (sda_conv_stats_rows: one per unit of the kernel
                                       the flags and the width route to — with SDA_CONV_FLAT_TILES and a Cout_p that divides by neither
                                       160 nor 128 that is the tile-per-workgroup kernel, B * n_t_tiles rows) = per-unit column
                                       sums of the products in plane 0 (the bias gradient of the layer that fed the GELU), plane 1
                                       zero.  No bias / y_pre / SDA_EPI_GELU */
       SDA_EPI_BN_STORE_DG = 262144,/* with bn_x (the BatchNorm-backward statistics epilogue): y = dg = round(dy) * GELU'(gamma * xhat + beta),
                                       rounded to the storage type, INSTEAD of dy, and the statistics are those of dg as stored —
                                       sda_bn_gelu_backward_from_stats_dg / _apply_dg then finish the BatchNorm backward without
                                       evaluating GELU' a second time */
       SDA_EPI_ROW_SUMSQ = 131072   /* the flat kernel-size-1 form only (SDA_CONV_FLAT_TILES must be set, else the call fails), Cout_p % 128 == 0: `stats` = float [>= B * (T + SDA_ROW_PAD) rows][Cout_p / 128]; entry
                                       [r][j] = sum of squares of buffer row r's output channels [128 j, 128 j + 128) as stored
                                       (rows that are padding are not written); sda_rows_sumsq_from_row_parts turns them into
                                       per-sample norms */ };

int sda_abi_version(void);
const char* sda_last_error(void);
long sda_rows_alloc(int B, int T);
int sda_pad_channels(int C);

/* (B, C, T) fp32 contiguous  ->  RL rows of Cp elements of `dtype` (channel padding zero-filled; pad
 * rows are NOT touched: the caller zero-initialises the buffer once). */
int sda_pack_rows(const float* src, void* dst, int B, int C, int T, int Cp, int dtype, void* stream);
/* the same with padding channel `ones_channel` (C <= ones_channel < Cp) set to 1 on every valid row: a bias folded into a
 * per-sample weight matrix rides on it (the composed SubjectBlock, models.py:111-117) */
int sda_pack_rows_ones(const float* src, void* dst, int B, int C, int T, int Cp, int ones_channel, int dtype, void* stream);
/* RL -> (B, C, T) fp32 contiguous */
int sda_unpack_rows(const void* src, float* dst, int B, int C, int T, int Cp, int dtype, void* stream);
/* RL of `dtype` -> (B, C, T) contiguous of `dst_dtype` (fp32 / bf16 / fp16): the loss's speech-embedding gradient in the
 * argument's own dtype (one rounding when dst_dtype is narrower than dtype) */
int sda_unpack_rows_typed(const void* src, void* dst, int B, int C, int T, int Cp, int dtype, int dst_dtype, void* stream);
/* (B, C, T) contiguous of `src_dtype` (fp32 / bf16 / fp16) -> RL rows of Cp elements of `dtype`, one pass (no widened fp32 copy):
 * the contract of sda_pack_rows — valid rows written with their channel padding zero-filled, pad rows NOT touched (the
 * destination is zero-initialised).  Host pointers, unknown dtypes and Cp < C are refused before any launch. */
int sda_pack_rows_typed(const void* src, void* dst, int B, int C, int T, int Cp, int src_dtype, int dtype, void* stream);

/* per-sample sum of squares over an RL tensor viewed as B rows of `row_elems` contiguous elements with
 * pitch `pitch` (elements). out[b] fp32. `scratch` holds B*64 floats. */
int sda_rows_sumsq(const void* x, float* out, float* scratch, int B, long row_elems, long pitch,
                   int dtype, void* stream);
/* the same norms for a tensor a conv just produced, from that conv's per-tile statistics ([B * tiles_per_sample][2][Cp],
 * plane 1 = sum of squares of the stored values): no second pass over the tensor */
int sda_rows_sumsq_from_stats(const float* stats, int tiles_per_sample, int Cp, float* out, int B, void* stream);
/* the same from SDA_EPI_ROW_SUMSQ's per-row partial sums ([rows][n_parts]): out[b] = sum over sample b's T rows and
 * n_parts entries, fp64, fixed order */
int sda_rows_sumsq_from_row_parts(const float* parts, int n_parts, float* out, int B, int T, void* stream);

/* fp32 conv weight [nW][Cout][Cin][KS]  ->  packed `dtype` operand.
 * mode 0 (forward):  dst[n][tap][co'][ci]  = w[n][co][ci][tap]
 * mode 1 (dgrad):    dst[n][tap][ci][co']  = w[n][co][ci][KS-1-tap]
 * co' = co if glu_half == 0, else (co < glu_half ? co : glu_half_p + (co - glu_half)).
 * Rows/cols beyond the source extent are zero. Cout_p/Cin_p are the padded extents of co'/ci. */
int sda_pack_conv_weight(const float* w, void* dst, int nW, int Cout, int Cin, int KS, int Cout_p,
                         int Cin_p, int mode, int glu_half, int glu_half_p, int dtype, void* stream);
/* All operand packs of a step in one launch.  `descs` is a DEVICE array of n descriptors: a weight pack as in
 * sda_pack_conv_weight (dst of `dtype`), or with is_vector != 0 a bias pack as in sda_pack_vector (Cout = C,
 * Cout_p = Cp, dst fp32).  total = number of destination elements; max_total = the largest of them. */
typedef struct sda_pack_desc {
  const float* src;
  void* dst;
  int nW, Cout, Cin, KS, Cout_p, Cin_p, mode, glu_half, glu_half_p, is_vector;
  int glu_tile;   /* 0: the two GLU halves stay contiguous ([0, glu_half_p) values, then gates); 80: SDA_EPI_GLU's layout —
                   * packed output channel 160 j + w is value channel 80 j + w (w < 80) or gate channel 80 j + w - 80 */
  long total;
} sda_pack_desc;
int sda_pack_multi(const sda_pack_desc* descs, int n, long max_total, int dtype, void* stream);
/* dst fp32 [Cout][Cin][KS] = ordered sum over nslabs K-split slabs [KS][Cout_p][Cin_p] (sda_wgrad_gemm output),
 * i.e. sda_reduce_slabs + sda_unpack_conv_wgrad in one pass */
int sda_reduce_unpack_wgrad(const float* slabs, int nslabs, float* dst, int Cout, int Cin, int KS, int Cout_p,
                            int Cin_p, int glu_half, int glu_half_p, void* stream);
/* Adam step (torch.optim.Adam defaults: no weight decay, no amsgrad; train.py:161-163) over n tensors in one
 * launch.  descs: DEVICE array; n = number of fp32 elements (complex parameters count their real view);
 * aligned != 0 when all four pointers are 16-byte aligned.  step = 1-based update count (bias correction). */
typedef struct sda_adam_desc {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long n;
  int aligned;
} sda_adam_desc;
int sda_adam_multi(const sda_adam_desc* descs, int n, long max_n, float lr, float beta1, float beta2, float eps,
                   long step, void* stream);
/* fp32 vector [C] -> padded fp32 [Cp] with the same GLU remap */
int sda_pack_vector(const float* v, float* dst, int C, int Cp, int glu_half, int glu_half_p, void* stream);
/* inverse of mode 0 for gradients: fp32 [nW][KS][Cout_p][Cin_p] -> fp32 [nW][Cout][Cin][KS] */
int sda_unpack_conv_wgrad(const float* g, float* dst, int nW, int Cout, int Cin, int KS, int Cout_p,
                          int Cin_p, int glu_half, int glu_half_p, void* stream);
int sda_unpack_vector(const float* g, float* dst, int C, int Cp, int glu_half, int glu_half_p, void* stream);

/* Implicit-GEMM 1-D convolution, kernel size 1 or 3, stride 1, "same" zero padding, dilation <= 16:
 *   y[b, t, co] = bias[co] + sum_{tap, ci} x[b, t + (tap - KS/2) * dil, ci] * w[widx[b]][tap][co][ci]  (+ res[b, t, co])
 * Serves the forward convolutions, the data gradients (weights packed with mode 1) and, with
 * ksplit > 1, the B x B similarity matmul of the loss (raw fp32 partial slabs, no epilogue). */
typedef struct sda_conv_args {
  const void* x;        /* RL [rows][x_pitch]; contraction over Cin_p elements of each row */
  const void* w;        /* packed [nW][KS][Cout_p][w_pitch] */
  const float* bias;    /* [Cout_p] or NULL */
  const void* res;      /* RL [rows][Cout_p] residual added in the epilogue, or NULL */
  void* y;              /* RL [rows][Cout_p] output (post-activation when SDA_EPI_GELU; [rows][Cout_p / 2] with SDA_EPI_GLU) */
  void* y_pre;          /* with SDA_EPI_GELU: pre-activation output, or NULL; with SDA_EPI_GLU: the gate, or NULL */
  const int32_t* widx;  /* [B] weight selector per sample (device), or NULL */
  float* stats;         /* [B * n_t_tiles][2][Cout_p] per-tile (sum, sum of squares) over valid rows, or NULL */
  float* partial;       /* ksplit > 1: [ksplit][T][Cout_p] fp32 raw accumulators (B must be 1) */
  const void* bn_x;     /* optional RL [rows][Cout_p]: input of the BatchNorm+GELU whose OUTPUT gradient this conv
                         * produces (data-gradient convs).  With bn_x, `stats` receives the per-tile sums of the
                         * BatchNorm backward instead: [tile][0][c] = sum dg, [tile][1][c] = sum dg * xhat, with
                         * dg = y * GELU'(gamma * xhat + beta), xhat = (bn_x - mean) * rstd, y as stored */
  const float* bn_coef; /* with bn_x: [4][Cout_p] = gamma, beta, mean, rstd (zero on padded channels) */
  const void* glu_out;  /* with SDA_EPI_GLU_BWD: RL [rows][Cout_p] forward output of the GLU (value * sigmoid(gate)) ... */
  const void* glu_gate; /* ... and its gate, RL [rows][Cout_p] */
  int B, T, Cin_p, Cout_p, KS, dil;
  long x_pitch, w_pitch; /* elements per row of x / per output-channel row of w.  With KS == 1, x_pitch < Cin_p is allowed:
                          * rows then overlap — a frame-major buffer read with pitch stride*C and row length k*C is the
                          * im2col matrix of a strided Conv1d (the wav2vec2 feature encoder) */
  long x_row0;           /* first row of sample 0 (SDA_ROW_PAD for RL, 0 for plain matrices) */
  long x_sample_rows;    /* rows between consecutive samples (T + SDA_ROW_PAD for RL) */
  long x_rows_limit;     /* rows >= limit read as zero */
  int w_rows_limit;      /* output channels >= limit read as zero (Cout_p when fully padded) */
  int ksplit;            /* >= 1 */
  int flags, dtype;
} sda_conv_args;
int sda_conv_gemm(const sda_conv_args* a, void* stream);
int sda_conv_n_t_tiles(int T);
/* output-channel tile (160 / 128 / 64) of the tile-per-workgroup kernels for Cout_p channels, kernel size KS, with or without a
 * `stats` buffer: what sda_conv_gemm dispatches on where sda_conv_kernel says SDA_CONV_KERNEL_TILE.  Host only. */
int sda_conv_tile_co(int Cout_p, int KS, int has_stats);
/* number of [2][Cout_p] rows of `stats` a launch with these parameters writes: one per unit of the kernel sda_conv_kernel names
 * (-1 where it refuses).  Host only. */
int sda_conv_stats_rows(int B, int T, int KS, int Cout_p, int flags);
/* the kernel sda_conv_gemm routes a convolution of kernel size KS and Cout_p output channels with these flags and storage type to:
 * TILE = one 128-row tile per workgroup (conv_gemm.hip), FLAT3 / FLAT1 = conv3_flat.hip / conv1_flat.hip, WIDE = conv1_wide.hip;
 * -1 (sda_last_error set) where the flags demand a kernel the shape or the storage type cannot have.  Host only. */
enum { SDA_CONV_KERNEL_TILE = 0, SDA_CONV_KERNEL_FLAT3 = 1, SDA_CONV_KERNEL_FLAT1 = 2, SDA_CONV_KERNEL_WIDE = 3 };
int sda_conv_kernel(int KS, int Cout_p, int flags, int dtype);

/* BatchNorm1d (training statistics) over valid rows.
 * finalize: per-tile partial (sum, sumsq) -> mean/rstd, fused affine scale/shift, running-stat update
 * (momentum, unbiased variance) when running_mean != NULL.  In eval mode call with ntiles = 0 and the
 * running stats: scale/shift are derived from them. */
int sda_bn_finalize(const float* partial, int ntiles, double count, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var, float* mean,
                    float* rstd, float* scale, float* shift, float* bwd_coef /* optional [4][Cp]: gamma, beta,
                    mean, rstd for sda_conv_args.bn_coef */, int C, int Cp, int training,
                    long* batches_tracked /* optional: the module's num_batches_tracked, += 1 in training mode */, void* stream);
/* y = GELU(x * scale[c] + shift[c]) on valid rows */
int sda_bn_gelu_forward(const void* x, void* y, const float* scale, const float* shift, int B, int T,
                        int Cp, int dtype, void* stream);
/* backward of y = GELU(BN(x)) (training statistics), two calls so that data-parallel ranks can
 * all-reduce the sums in between:  dg = dy * GELU'(u);
 * reduce: dbeta = sum dg, dgamma = sum dg*xhat over this rank's valid rows (fp32 [Cp]; ordered
 *         two-stage reduction through `partial`, sda_reduce_scratch_floats(Cp) floats);
 * apply:  dx = gamma*rstd*(dg - dbeta/count - xhat*dgamma/count), count = GLOBAL number of rows. */
int sda_bn_gelu_backward_reduce(const void* dy, const void* x, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, int C, float* partial, float* dgamma,
                                float* dbeta, int B, int T, int Cp, int dtype, void* stream);
/* out0[c] = sum_k partial[k][0][c] (and out1 from [k][1][c] when out1 != NULL): fixed-order fp64 reduction of
 * per-tile statistics written by sda_conv_gemm (`stats`), e.g. the BatchNorm backward sums of bn_x mode. */
int sda_reduce_stats(const float* partial, int nrows, float* out0, float* out1, int Cp, void* stream);
/* Single-process shortcut: per-tile sums (sda_conv_gemm bn_x mode) -> dgamma/dbeta + coefficient table in ONE
 * launch, then the apply pass.  (Data-parallel runs use sda_reduce_stats, all-reduce the two sums, then ..._apply.) */
int sda_bn_gelu_backward_from_stats(const float* partial, int nrows, const void* dy, const void* x, const float* mean,
                                    const float* rstd, const float* gamma, const float* beta, int C, double count,
                                    float* dgamma, float* dbeta, float* coef, void* dx, int B, int T, int Cp, int dtype,
                                    void* stream);
int sda_bn_gelu_backward_apply(const void* dy, const void* x, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, int C, const float* dgamma,
                               const float* dbeta, double count, float* coef /* 6*Cp floats scratch */, void* dx,
                               int B, int T, int Cp, int dtype, void* stream);
/* the same two for a gradient buffer that already holds dg = dy * GELU'(gamma * xhat + beta) (written by sda_conv_gemm with
 * SDA_EPI_BN_STORE_DG, whose statistics rows are those of dg as stored): no second GELU' evaluation */
int sda_bn_gelu_backward_from_stats_dg(const float* partial, int nrows, const void* dy, const void* x, const float* mean,
                                    const float* rstd, const float* gamma, const float* beta, int C, double count,
                                    float* dgamma, float* dbeta, float* coef, void* dx, int B, int T, int Cp, int dtype,
                                    void* stream);
int sda_bn_gelu_backward_apply_dg(const void* dy, const void* x, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, int C, const float* dgamma,
                               const float* dbeta, double count, float* coef /* 6*Cp floats scratch */, void* dx,
                               int B, int T, int Cp, int dtype, void* stream);

int sda_reduce_scratch_floats(int Cp);

/* Zero the rows of an RL buffer that kernels never write: the SDA_ROW_PAD rows in front of each of the B samples and the
 * slack behind the last one (a buffer whose valid rows a kernel is about to fill needs nothing else initialised) */
int sda_zero_pad_rows(void* buf, int B, int T, int Cp, int dtype, void* stream);
/* nbytes zero bytes at p (16-byte aligned): the fresh zero gradients a backward hands out (conv biases in front of a training-mode
 * BatchNorm: autograd's zero, speech_decoding/models.py:135,143) without a framework fill kernel in the step */
int sda_fill_zero(void* p, long nbytes, void* stream);
/* dst sample b = table sample idx[b] (idx: B int64 on the device), samples of sample_bytes contiguous bytes (a multiple of 16).
 * The resident-feed form of `Y = dataset.Y[batch indices]` (gwilliams2022.py:129-142 hands out one embedding per item): with the
 * embedding table kept in row layout (a sample = (T + SDA_ROW_PAD) * Cp elements, pad rows included) the gathered batch IS the
 * packed row-layout operand of the loss — no index_select + sda_pack_rows pair per step */
int sda_gather_samples(const void* table, const long* idx, void* dst, int B, long sample_bytes, void* stream);
/* The same batch gathered from WINDOWS of a table of plain rows (retrieval.WindowBank.table: table_rows rows of row_bytes bytes,
 * row_bytes = pad64(F) * element size, a multiple of 128; the kernel moves bytes, so one serves bf16, fp16 and fp32):
 *     dst sample b = SDA_ROW_PAD zero rows, then table rows starts[idx[b]] ... starts[idx[b]] + T - 1, bit for bit
 * starts: M device int32 table rows; idx: B device int64 candidates in [0, M), any order, duplicates allowed; dst: a row-layout
 * buffer of sda_rows_alloc(B, T) rows of row_bytes bytes.  ONE launch writes every byte of dst — the pad rows, the windows with
 * the table's (zero) channel padding and the slack behind the last sample — so dst may arrive uninitialised, no sda_zero_pad_rows
 * launch goes with it, and the result IS the packed row-layout operand of the loss: a track is stored once however many
 * overlapping windows are cut from it (gwilliams2022.py materialises every window of the speech side).  Nothing outside the
 * table is read: an idx[b] outside [0, M) or a start outside [0, table_rows - T] gives a sample of zeros and touches nothing
 * else.  Fixed order, no atomics.  Refused before any launch: null pointers; B, T or M < 1; B > 65535; table_rows < T; row_bytes
 * not a multiple of 128; table or dst not 16-byte aligned. */
int sda_gather_windows(const void* table, long table_rows, const int32_t* starts, int M, const long* idx, void* dst, int B, int T,
                       long row_bytes, void* stream);
/* out[i] = a[i] * b[0], i < n (device scalars: e.g. d loss / d temp times the incoming gradient) */
int sda_scalar_mul(const float* a, const float* b, float* out, int n, void* stream);

/* GLU over channels: y[:, c] = x[:, c] * sigmoid(x[:, Ch + c]), x has 2*Ch channels (models.py:164) */
int sda_glu_forward(const void* x, void* y, int B, int T, int Ch, int dtype, void* stream);
int sda_glu_backward(const void* x, const void* dy, void* dx, int B, int T, int Ch, int dtype, void* stream);
/* du = dz * GELU'(u) */
int sda_gelu_backward(const void* u, const void* dz, void* du, int B, int T, int Cp, int dtype, void* stream);
/* the same two backward stages fused with the column sums of their own output (= the bias gradient of the
 * layer that produced x / u): colsum fp32 [2*Ch] resp. [Cp]; scratch sda_reduce_scratch_floats(.) floats */
/* (colsum == NULL: the final reduction is left to the caller — scratch then holds sda_reduce_scratch_rows(B, T) rows of
 * [2][Ch] (resp. [2][Cp], slot 1 unused) partial sums for sda_reduce_stats, e.g. on another stream) */
int sda_reduce_scratch_rows(int B, int T);
int sda_glu_backward_colsum(const void* x, const void* dy, void* dx, float* colsum, float* scratch, int B, int T,
                            int Ch, int dtype, void* stream);
int sda_gelu_backward_colsum(const void* u, const void* dz, void* du, float* colsum, float* scratch, int B, int T,
                             int Cp, int dtype, void* stream);
/* GLU backward after a forward with SDA_EPI_GLU (the value half was never stored): out = value * sigmoid(gate) and gate,
 * both RL [rows][Ch]; dx RL [rows][2*Ch] = [d value | d gate] = [dy * sig(g) | dy * out * (1 - sig(g))]; colsum as above */
int sda_glu_backward_colsum_og(const void* out, const void* gate, const void* dy, void* dx, float* colsum, float* scratch,
                               int B, int T, int Ch, int dtype, void* stream);
/* column sums of an RL tensor over valid rows: out[c] = sum_{b,t} x[b,t,c]  (bias gradients) */
int sda_colsum(const void* x, float* out, float* scratch /* sda_reduce_scratch_floats(Cp) */, int B, int T,
               int Cp, int dtype, void* stream);

/* Weight-gradient GEMM:  g[seg][tap][co][ci] = sum_{b in seg} sum_t dy[b,t,co] * x[b, t+(tap-KS/2)*dil, ci]
 * Samples are visited through `perm` (device int32 [B]); segment s covers perm[seg_start[s]..seg_start[s+1]).
 * Output fp32 slabs [nseg][KS][Cout_p][Cin_p].  With out_e != NULL (KS must be 1, nseg 1) the result is
 * written as `dtype` rows instead:  out_e[co][ci] = out_scale * (acc_scale[co] * acc - rscale[co] * sub[co][ci])   (loss backward dZ). */
/* sda_wgrad_args.flags */
enum { SDA_WGRAD_FLAT_ROWS = 1  /* dy is a row-layout buffer whose rows between samples (the SDA_ROW_PAD rows in front of every
                                   sample, the slack behind the last) are zero.  perm == NULL: a segment is contracted as ONE run of
                                   rows, pad rows included (they contribute nothing), in whole K-chunks — no partial chunk per
                                   sample.  perm != NULL (ABI 4): every SAMPLE is extended into the zero rows around it to whole
                                   K-chunks (when (T rounded up to the chunk) - T <= 2 * SDA_ROW_PAD; ignored otherwise) */ };
typedef struct sda_wgrad_args {
  const void* dy;       /* RL [rows][dy_pitch] */
  const void* x;        /* RL [rows][x_pitch] */
  float* g;             /* [nseg][KS][Cout_p][Cin_p] fp32 */
  void* out_e;          /* optional typed output [Cout rows][out_pitch] */
  const void* sub;      /* optional [Cout rows][out_pitch] */
  const float* rscale;  /* optional [Cout] */
  const float* out_scale; /* optional device scalar multiplying the typed output (incoming dloss) */
  const int32_t* perm;
  const int32_t* seg_start; /* device int32 [nseg + 1] */
  int nseg, B, T, Cout_p, Cin_p, KS, dil;
  long dy_pitch, x_pitch, out_pitch;
  long row0, sample_rows; /* as in sda_conv_args */
  long rows_limit;        /* x rows are clamped into [0, rows_limit) (they only meet zero dy rows out there) */
  long dy_zero_row;       /* index of a row of dy that is all zero (row 0 of any RL buffer); stands in for t >= T */
  int co_valid;           /* rows of out_e to write (out_e mode) */
  int dtype;
  const float* acc_scale; /* optional [Cout]: multiplies the fp32 accumulator of typed-output row co before `sub` is taken off */
  int flags;              /* SDA_WGRAD_FLAT_ROWS */
} sda_wgrad_args;
int sda_wgrad_gemm(const sda_wgrad_args* a, void* stream);
/* output-channel (row) tile (160 / 128 / 64) sda_wgrad_gemm dispatches on for Cout_p channels.  Host only. */
int sda_wgrad_tile_m(int Cout_p);
/* dst[i] = sum_s src[s][i] in fixed order */
int sda_reduce_slabs(const float* src, float* dst, int nslabs, long n, void* stream);
/* The loss's similarity matmul (loss.py:68) on 256 x 256 output tiles, 16-bit storage (csrc/sim_gemm.hip):
 *     partial[ks][i][j] = sum_{k in K slice ks} X[i][k] * W[j][k],   i < M, j < Np, ks < ksplit      (fp32)
 * X (M rows) and W (N rows) are K-contiguous rows `pitch` elements apart (K % 32 == 0, 16-byte aligned); columns [N, Np) are
 * don't-care.  The caller sums the K slices with sda_reduce_slabs (fixed order).  sda_sim_gemm_ksplit returns the number of
 * K slices to launch with for this shape on the current device, 0 if the shape is not served (fp32 storage: use sda_conv_gemm's
 * split-K matrix mode). */
int sda_sim_gemm_ksplit(int M, int N, long K, int dtype);
int sda_sim_gemm(const void* X, const void* W, float* partial, int M, int N, int Np, long K, long pitch, int ksplit, int dtype,
                 void* stream);
/* The same product against WINDOWS of a table of plain rows (decoding against continuous speech tracks, retrieval.WindowBank):
 *     partial[ks][i][j] = sum_{k in K slice ks} X[i][k] * table[starts[j] * row_elems + k],   i < M, j < Np, ks < ksplit
 * Candidate j is the K = T * row_elems elements from table row starts[j] on, so candidates that overlap share their bytes.
 * X: M rows x_pitch elements apart (x_pitch >= K, x_pitch % 8 == 0); table: rows of row_elems (% 64 == 0) elements; starts:
 * N device int32 table rows; base_row: the smallest of them — the kernel addresses a candidate as the wave-uniform base
 * table + base_row * row_elems plus a 32-bit byte offset, so the CALLER (who holds the starts on the host) guarantees
 *     0 <= starts[j] - base_row <= sda_sim_gemm_windows_span(row_elems)        for every j < N
 * and that every window lies inside the table; a start that breaks the first promise is clamped into it (a wrong score, no
 * wrapped address).  Reads stay inside the windows named by starts[0, N): columns past N repeat the last candidate and are
 * don't-care in [N, Np).  16-bit storage only: there is no fp32 window path.  Tiles, K slices (sda_sim_gemm_ksplit(M, N, K))
 * and the slab sum (sda_reduce_slabs) are sda_sim_gemm's.  Refused before any launch: null pointers, fp32, K % 32, row_elems
 * % 64, x_pitch < K or % 8, Np < N or % 4, ksplit outside [1, K / 32], base_row < 0, X / table / partial not 16-byte aligned. */
int sda_sim_gemm_windows(const void* X, long x_pitch, const void* table, const int32_t* starts, int base_row, long row_elems,
                         float* partial, int M, int N, int Np, long K, int ksplit, int dtype, void* stream);
/* largest starts[j] - base_row one sda_sim_gemm_windows launch serves (0: row_elems is not a positive multiple of 64).  Host only. */
long sda_sim_gemm_windows_span(long row_elems);
/* Squared norms of such windows from the per-row sums of the table (row_sq[l] = sum of squares of table row l, fp32:
 * sda_rows_sumsq over rows of row_elems elements):  out[m] = sum_{t < T} row_sq[starts[m] + t],  m < M.  One wavefront per
 * candidate: lane l adds t = l, l + 64, ... in order, then the xor butterfly (sda_gather_baseline_windows' order): no atomics,
 * the same bits on every call.  The caller guarantees starts[m] + T <= rows of row_sq.  Null pointers, M < 1, T < 1 refused. */
int sda_window_sumsq(const float* row_sq, const int32_t* starts, float* out, int M, int T, void* stream);

/* SpatialAttention weights (models.py:49-58 with SpatialDropout 81-84 folded in):
 * a = Re(z) cos + Im(z) sin; W = softmax_c(a); Wd = W * mask.  z is complex64 interleaved (re, im).
 * Outputs: W fp32 [D1][C] (saved for backward) and the packed operand Wp `dtype` [D1p][Cp]. */
int sda_sa_weights_forward(const float* z, const float* cos_t, const float* sin_t, const float* mask,
                           float* W, void* Wp, float* scratch /* sda_sa_scratch_floats(D1, K2, C) */, int D1, int K2,
                           int C, int D1p, int Cp, int dtype, void* stream);
int sda_sa_scratch_floats(int D1, int K2, int C);
/* The same weight build with its two contractions on the matrix cores (sda_conv_gemm in split-K matrix mode, fp32):
 * forward  a (D1 x C, pitch a_pitch) = [Re z | Im z] . [cos | sin]^T, then sda_sa_softmax_pack = softmax over sensors,
 *          dropout mask, W fp32 and the packed operand Wp (as sda_sa_weights_forward);
 * backward sda_sa_softmax_backward: da = W (dWd*mask - <dWd*mask, W>) (D1 x da_pitch, padding zeroed), then
 *          dz = da . [cos ; sin] by the same GEMM. */
int sda_sa_softmax_pack(const float* a, int a_pitch, const float* mask, float* W, void* Wp, int D1, int C, int D1p,
                        int Cp, int dtype, void* stream);
int sda_sa_softmax_backward(const float* dWd, int dwd_pitch, const float* W, const float* mask, float* da,
                            int da_pitch, int D1, int C, void* stream);
/* dWd fp32 [D1p][Cp] (from sda_wgrad_gemm) -> dz complex64 interleaved [D1][K2].
 * cosT/sinT are the transposed tables [C][K2] (constant buffers, transposed once by the host).  C <= 512 and C <= Cp. */
int sda_sa_weights_backward(const float* dWd, const float* W, const float* mask, const float* cosT,
                            const float* sinT, float* dz, int D1, int K2, int C, int Cp, void* stream);

/* CLIP loss tail on the raw similarity S[i][j] = <Y_i, Z_j> (rows = speech, loss.py:60-79):
 * logits = S / (|Y_i| |Z_j|) * exp(temp); per-row (max, sumexp) over the local column block, per-column
 * lse over all rows, and diag[i] = logits[i][i - col0] for rows whose positive lives in this block.
 * Multi-GPU: rows are global (Bm), columns are this rank's Bn samples starting at global index col0;
 * zsq holds the Bn local norms. */
int sda_clip_logits_stats(const float* S, long s_pitch, const float* ysq, const float* zsq, const float* temp,
                          float* logits, float* row_max, float* row_sum, float* col_lse, float* diag /* every row written: 0 where
                          the positive lives elsewhere */, float* row_lse /* optional: max + log(sum) of the local block */,
                          int Bm, int Bn, int col0, void* stream);
/* Given the final row lse (after any cross-rank merge), with D_ij = p_row + p_col - 2 delta (dloss/dlogits = inv_norm * D):
 * G[i][j] = D_ij * ymax / |Y_i| (ymax = max_i |Y_i|: O(1) entries, safe in 16-bit) stored as `dtype` with pitch g_pitch —
 * [Bm + 1][g_pitch], the extra row and the columns >= Bn are written as zeros —, cscale[j] = inv_norm * exp(temp) /
 * (ymax |Z_j|) (the factor taken out of G: sda_wgrad_args.acc_scale of the dZ product), rscale[j] = inv_norm * sum_i D_ij
 * logits_ij / |Z_j|^2, so that dZ_j = cscale_j * sum_i G_ij Y_i - rscale_j Z_j; scalars[0] = this block's share of the loss,
 * scalars[1] = its share of dloss/dtemp.  inv_norm = 1/(2*B_global) for reduction="mean", 1/2 for "sum".  colpart: 2*Bn floats.
 * The block's positives are rows of it: 0 <= col0 and col0 + Bn <= Bm, or the call is refused. */
int sda_clip_grad(const float* logits, const float* row_lse, const float* col_lse, const float* ysq,
                  const float* zsq, const float* temp, float inv_norm, int col0, void* G, long g_pitch,
                  float* rscale, float* cscale, float* colpart, float* scalars, int Bm, int Bn, int dtype, void* stream);
/* The coefficients of the loss's gradient with respect to the SPEECH embeddings (the first argument), the dZ product with the
 * two roles exchanged:  dY_i = cscale_y_i * sum_j Gy[j][i] * Z_j - rscale_y_i * Y_i.  On one logits block (rows = speech i,
 * columns = this block's brain j; same logits / row_lse / col_lse / col0 as sda_clip_grad, D_ij from the same expression):
 * Gy[j][i] = D_ij * zmax / |Z_j| as `dtype`, [Bn + 1][gy_pitch] with the row Bn and every unused column written as zeros;
 * zmax = max over the nz norms zsq_all (all brain rows the dY GEMM contracts over: the gathered ones under data parallelism).
 * Column c holds speech row (c / seg_pitch) * seg + c % seg (c % seg_pitch < seg; seg_pitch a multiple of 64, gy_pitch a
 * multiple of seg_pitch): seg = Bm, seg_pitch = gy_pitch = pad64(Bm) on one GPU, one 64-aligned group per rank's rows under
 * data parallelism.  part [ceil(Bn / 64)][Bm] fp32: per-row partial sums of D_ij * logits_ij over 64-column groups. */
int sda_clip_grad_y(const float* logits, const float* row_lse, const float* col_lse, const float* zsq,
                    const float* zsq_all, int nz, int col0, void* Gy, long gy_pitch, int seg, int seg_pitch,
                    float* part, int Bm, int Bn, int dtype, void* stream);
/* rows [row0, row0 + nrows) of the dY factors: rscale_y[r] = inv_norm * sum_p part[p][i] / |Y_i|^2 and cscale_y[r] = inv_norm *
 * exp(temp) / (zmax |Y_i|), i = row0 + r, from nparts rows of [Bg] partials (the blocks of every rank in rank order, summed in
 * that order: the same bits on every rank and every call).  Then sda_clip_dz(Gy, g_pitch, Z, Y, dY, cscale_y, rscale_y, ...)
 * with Bm = the brain rows contracted over and Bn = nrows gives dY. */
int sda_clip_grad_y_finish(const float* part, int nparts, int Bg, const float* ysq, const float* zsq_all, int nz,
                           const float* temp, float inv_norm, int row0, int nrows, float* rscale_y, float* cscale_y,
                           void* stream);
/* The embedding gradient of the loss on one GPU as a streaming kernel (loss_gemm.hip):
 *     out[j][k] = out_scale[0] * (cscale[j] * sum_{i < Bm} G[i][j] * Y[i][k] - rscale[j] * Z[j][k]),   j < Bn, k < row_elems
 * G [Bm][g_pitch], Y [Bm][row_elems], Z and out [Bn][row_elems] of `dtype` (16-bit types only), cscale / rscale fp32 [Bn]
 * (cscale may be NULL = 1), out_scale a device scalar or NULL.  Same result as sda_wgrad_gemm's typed-output mode, which
 * serves what this one does not: sda_clip_dz_supported() says whether a shape is served — bf16 / fp16 and either
 * Bm <= 256 with row_elems % 64 == 0 (the coefficient matrix in registers) or, ABI 4, Bm >= 256 with Bm % 32 == 0,
 * row_elems % 256 == 0 and g_pitch % 8 == 0 (256 x 256 tiles: any number of speech rows — a rank's block under data
 * parallelism contracts over the GLOBAL batch, loss.py:68 with x all-gathered). */
int sda_clip_dz_supported(int Bm, int Bn, long row_elems, int dtype);
int sda_clip_dz(const void* G, long g_pitch, const void* Y, const void* Z, void* out, const float* cscale, const float* rscale,
                const float* out_scale, int Bm, int Bn, long row_elems, int dtype, void* stream);
/* Extra speech NEGATIVES for the loss, read in place from a table of plain rows (csrc/clip_negatives.hip; ABI 4, additions):
 * negative n < N is the K = T * row_elems elements from table row starts[n] on (retrieval.WindowBank), with squared norm wsq[n].
 * It has no brain partner: m_nj = <W_n, Z_j> exp(temp) / (|W_n| |Z_j|) joins the column (brain -> speech) soft-max only, there
 * is no row term and no gradient into the table.  The raw scores S[j][n] = <Z_j, W_n> (brain-major, s_pitch >= N) come from
 * sda_sim_gemm_windows with the brain rows as X.  16-bit storage only, no atomics, every sum in an order fixed by the shape.
 * sda_clip_neg_stats: mlog fp32 [Bn][N] = m_nj (sda_clip_logits_stats' expression), and col_lse[j] <- logaddexp(col_lse[j],
 * lse_n m_nj) IN PLACE — between sda_clip_logits_stats(_masked) and sda_clip_grad(_labels) / sda_clip_grad_y(_labels), which
 * then compute the loss and the paired coefficients against the widened column soft-max without another term.
 * sda_clip_neg_grad (after sda_clip_grad on the same stream), D_nj = exp(m_nj - col_lse[j]):
 *   Gn[n][j] = D_nj wmax / |W_n| (wmax = max_n |W_n|) as `dtype`, [sda_clip_neg_rows(N)][g_pitch]: the rows from N on and the
 *   columns >= Bn are written as zeros; cscale_n[j] = inv_norm exp(temp) / (wmax |Z_j|); rscale[j] += inv_norm sum_n D_nj m_nj
 *   / |Z_j|^2 and scalars[1] += inv_norm sum_nj D_nj m_nj — one writer each; colpart: Bn floats of scratch.
 * sda_clip_neg_rows(N): N rounded up to whole 32-row K-steps, the rows Gn is allocated and read with. */
int sda_clip_neg_stats(const float* S, long s_pitch, const float* wsq, const float* zsq, const float* temp, float* mlog,
                       float* col_lse, int Bn, int N, void* stream);
int sda_clip_neg_rows(int N);
int sda_clip_neg_grad(const float* mlog, const float* col_lse, const float* wsq, const float* zsq, const float* temp,
                      float inv_norm, void* Gn, long g_pitch, float* cscale_n, float* rscale, float* colpart, float* scalars,
                      int Bn, int N, int dtype, void* stream);
/* The negatives' part of the brain-side gradient, added to what sda_clip_dz wrote (row-layout `out`: sample j is out_pitch
 * elements, its data behind SDA_ROW_PAD pad rows of row_elems):
 *     out[j][SDA_ROW_PAD * row_elems + k] += out_scale[0] * cscale_n[j] * sum_{n < N} Gn[n][j] * table[starts[n] * row_elems + k]
 * for j < Bn, k < K; nothing else of `out` is touched (pad rows and slack keep their bytes), each element has one writer.
 * 256 x 256 tiles of (j, k) over 32-row K-steps of negatives; N, Bn and K / 256 need not be whole tiles.  A negative is
 * addressed as the wave-uniform base table + base_row * row_elems plus a 32-bit byte offset: the CALLER (who holds the starts
 * on the host) guarantees 0 <= starts[n] - base_row <= span_rows <= sda_clip_dz_windows_span(row_elems) = (2^31 - 256) /
 * row_elems and that every window lies inside the table; a start that breaks the first promise is clamped into the span (a
 * wrong sum, no wrapped address).  Reads stay inside the windows named by starts[0, N).  Refused before any launch: null
 * pointers (out_scale may be NULL = 1); fp32; N, Bn < 1; K % 32 != 0 or K not whole table rows; row_elems % 64 != 0;
 * base_row < 0; g_pitch < Bn or % 8; out_pitch < SDA_ROW_PAD * row_elems + K or % 8; span_rows outside [0, the span]; Gn, table
 * or out not 16-byte aligned, starts not 4-byte aligned. */
long sda_clip_dz_windows_span(long row_elems);
int sda_clip_dz_windows(const void* Gn, long g_pitch, const void* table, const int32_t* starts, int base_row, long span_rows,
                        long row_elems, void* out, long out_pitch, const float* cscale_n, const float* out_scale, int N, int Bn,
                        long K, int dtype, void* stream);
/* cnt[i] = #{local j : logits[i][j] beats diag[i]} (ties: lower global index wins) — Classifier ranks */
int sda_clip_ranks(const float* logits, const float* diag, int32_t* cnt, int Bm, int Bn, int col0, void* stream);
/* The loss tail with speech labels (csrc/clip_labels.hip): samples of the global batch that carry the same speech segment are
 * matches of one another, not negatives.  labels: device int32 [Bg = Bm], one per global sample (row i: labels[i], local column
 * j: labels[col0 + j]); same_ij = (labels[i] == labels[j]), n_i = sum_j same_ij (sda_clip_label_counts: counts[i], exact).
 * Every entry point is its unlabelled sibling's twin in shapes, layouts, scaling and the order of its sums, and needs
 * 0 <= col0, col0 + Bn <= Bm.  mode:
 *   SDA_CLIP_DUP_POSITIVE  targets T_ij = same_ij / n_i: D_ij = p_row + p_col - 2 T_ij on the statistics of
 *                          sda_clip_logits_stats; scalars[0] sums (row_lse[col0 + j] - pbar_j) + (col_lse[j] - pbar_j) with
 *                          pbar_j = (1 / n_j) sum_i same_{i, col0 + j} logits_ij.
 *   SDA_CLIP_DUP_MASK      entries with same_ij, i != j leave both soft-max denominators (sda_clip_logits_stats_masked: they are
 *                          skipped in the row (max, sum) and in the column lse; the stored logits stay unmasked) and have
 *                          D_ij = 0; elsewhere D_ij = p'_row + p'_col - 2 delta_ij and the loss terms are the unlabelled ones.
 * sda_clip_ranks_labels counts only columns of another label: a repeat of the row's own speech is never a wrong answer. */
enum { SDA_CLIP_DUP_POSITIVE = 0, SDA_CLIP_DUP_MASK = 1 };
int sda_clip_label_counts(const int32_t* labels, int32_t* counts, int Bg, void* stream);
int sda_clip_logits_stats_masked(const float* S, long s_pitch, const float* ysq, const float* zsq, const float* temp,
                                 const int32_t* labels, float* logits, float* row_max, float* row_sum, float* col_lse,
                                 float* diag, float* row_lse, int Bm, int Bn, int col0, void* stream);
int sda_clip_grad_labels(const float* logits, const float* row_lse, const float* col_lse, const float* ysq,
                         const float* zsq, const float* temp, const int32_t* labels, const int32_t* counts, int mode,
                         float inv_norm, int col0, void* G, long g_pitch, float* rscale, float* cscale, float* colpart,
                         float* scalars, int Bm, int Bn, int dtype, void* stream);
int sda_clip_grad_y_labels(const float* logits, const float* row_lse, const float* col_lse, const float* zsq,
                           const float* zsq_all, int nz, const int32_t* labels, const int32_t* counts, int mode, int col0,
                           void* Gy, long gy_pitch, int seg, int seg_pitch, float* part, int Bm, int Bn, int dtype,
                           void* stream);
int sda_clip_ranks_labels(const float* logits, const float* diag, const int32_t* labels, int32_t* cnt, int Bm, int Bn,
                          int col0, void* stream);
/* The pairwise sigmoid loss tail (csrc/sigmoid_loss.hip) on the same raw similarity block S (rows = the Bm global speech samples,
 * columns = this block's Bn brain samples from global index col0; 0 <= col0, col0 + Bn <= Bm):
 *     a_ij = S_ij exp(temp) / (|Y_i| |Z_j|)   (the expression, and the bits, of sda_clip_logits_stats' logits),  l_ij = a_ij + bias,
 *     z_ij = +1 where i == col0 + j, else -1;  loss = inv_norm * sum_ij softplus(-z_ij l_ij);  D_ij = -z_ij sigma(-z_ij l_ij).
 * labels (device int32 [Bm], or NULL: then mode is ignored): a pair of two samples with one label has z = +1
 * (SDA_CLIP_DUP_POSITIVE) or is dropped (SDA_CLIP_DUP_MASK: no loss term, D_ij = 0 exactly).  inv_norm = 1 / B_global for
 * reduction="mean", 1 for "sum".  softplus and sigma are the stable forms: past |l| = 104 the term is |l| or 0 and D is -+1 or 0.
 * sda_sigmoid_pairs, one pass over the block: a fp32 [Bm][Bn]; diag as sda_clip_logits_stats writes it (every row; 0 where the
 * positive lives in another block); G[i][j] = D_ij ymax / |Y_i| as `dtype`, [Bm + 1][g_pitch] with row Bm and the columns >= Bn
 * written as zeros (sda_clip_grad's G); part fp32 [ceil(Bm / 64)][Bn][3] = (sum softplus, sum D a, sum D) of column j over
 * each group of 64 rows.
 * sda_sigmoid_finish (nparts = ceil(Bm / 64)) sums them in group order: rscale[j] = inv_norm * sum_i D_ij a_ij / |Z_j|^2,
 * cscale[j] = inv_norm * exp(temp) / (ymax |Z_j|) — so that sda_clip_dz gives dZ_j = cscale_j sum_i G_ij Y_i - rscale_j Z_j —
 * and scalars[3] = this block's shares of (loss, d loss / d temp, d loss / d bias), summed over the columns in fp64.
 * sda_sigmoid_grad_y is sda_clip_grad_y's twin (same Gy layout with seg / seg_pitch, zero row Bn, part [ceil(Bn / 64)][Bm] =
 * sums of D_ij a_ij): Gy[j][i] = D_ij zmax / |Z_j|, D from a, bias and the labels as above; its outputs go to
 * sda_clip_grad_y_finish and sda_clip_dz.  No atomics: every sum's order is fixed by the shape. */
int sda_sigmoid_pairs(const float* S, long s_pitch, const float* ysq, const float* zsq, const float* temp,
                      const float* bias, const int32_t* labels, int mode, int col0, float* a, float* diag, void* G,
                      long g_pitch, float* part, int Bm, int Bn, int dtype, void* stream);
int sda_sigmoid_finish(const float* part, int nparts, const float* ysq, const float* zsq, const float* temp,
                       float inv_norm, float* rscale, float* cscale, float* scalars, int Bm, int Bn, void* stream);
int sda_sigmoid_grad_y(const float* a, const float* bias, const float* zsq, const float* zsq_all, int nz,
                       const int32_t* labels, int mode, int col0, void* Gy, long gy_pitch, int seg, int seg_pitch,
                       float* part, int Bm, int Bn, int dtype, void* stream);
/* Decoding against a candidate bank (csrc/retrieval.hip): top-k selection over the raw fp32 dot products of n query rows
 * against M candidates, one pass over the matrix.  score[i][j] = S[i][j] / max(sqrt(qsq[i]) * sqrt(csq[j]), 1e-8) (the
 * similarity of models.py:223-232; a zero row scores 0), ordered by score descending, on equal scores the lower j first
 * (sda_clip_ranks' tie rule):
 *     indices[i][r], scores[i][r]  (r < k, [n][k] int64 / fp32) = the k best candidates of row i, best first
 *     ranks[i] (int32)             = #{j : j beats labels[i]} under the same order over all M columns (0 = top-1); -1 where
 *                                    labels[i] lies outside [0, M).  labels (device int64 [n]) and ranks are both given or both NULL.
 * S is CHUNK-MAJOR: columns come in chunks of `chunk_cols` (a multiple of 64); chunk c is a dense [n][pad64(its columns)]
 * matrix at float offset c * n * chunk_cols — the output of one similarity GEMM per bank chunk (sda_sim_gemm / sda_conv_gemm
 * split-K + sda_reduce_slabs).  chunk_cols >= M is the plain [n][pad64(M)] matrix; padding columns are ignored.
 * sda_retrieval_scores_floats gives the number of floats S holds (-1: bad arguments).  1 <= k <= min(64, M); S 16-byte
 * aligned.  Null pointers and out-of-range sizes are refused before any launch.  Deterministic. */
long sda_retrieval_scores_floats(int n, int M, int chunk_cols);
int sda_retrieval_select(const float* S, const float* qsq, const float* csq, const int64_t* labels, int64_t* indices,
                         float* scores, int32_t* ranks, int n, int M, int k, int chunk_cols, void* stream);
/* Class-level decoding on the same matrix: the M candidates fall into C classes (words), given as a CSR index built on the
 * host — order[M], the candidates sorted by class (ascending candidate index inside a class), and offsets[C + 1]; class c owns
 * order[offsets[c] ... offsets[c + 1]) and may be empty.  With the logit l[i][j] = scale * score[i][j] (score as above, the
 * product rounded once to fp32), sda_retrieval_class_reduce writes for every row i < n and class c < C
 *     out[i * out_pitch + c] = f(i, c) - row_lse[i]
 *     mode 0 "sum":  f = m + log sum_{j in c} exp(l[i][j] - m), m = max_{j in c} l[i][j] — the class's OWN maximum, so a class
 *                    far below the row's best one keeps its value instead of underflowing to -inf
 *     mode 1 "mean": the "sum" value - log(members of c)         mode 2 "max": m         an empty class: -inf in every mode
 *     row_lse[i]   = log-sum-exp over the classes, in class order, of the "sum" values = log sum_j exp(l[i][j])
 * so "sum" gives log-probabilities that sum to one over the classes.  Columns c >= C of a row (out_pitch >= C) are NOT written.
 * S, qsq, csq, n, M, chunk_cols as for sda_retrieval_select.  expf / logf at full precision; every sum is taken in an order
 * fixed by (order, offsets) alone — a class of up to 256 members by 8 adjacent lanes (lane a: members a, a + 8, ...; xor tree
 * 4, 2, 1), a larger one by the 1024 threads of the row's workgroup (thread t: members t, t + 1024, ...; xor tree inside each
 * wave, then the waves in order) — and there are no floating-point atomics: the same call gives the same bits.  An index of
 * `order` outside [0, M) is clamped into the bank, offsets are clamped into [0, M]: nothing is read past the row.
 * sda_retrieval_pool_rows pools rows that are repetitions of one item: group g owns rows[group_offsets[g] ...
 * group_offsets[g + 1]) (the same CSR form, G groups over N rows, built on the host) and
 *     out[g * out_pitch + c] = log( (1 / members of g) * sum_{r in g} exp(V[r * v_pitch + c]) ),   c < C,
 * rows in list order, with the column's own maximum; a column that is -inf in every row of the group (and an empty group)
 * gives -inf, never NaN.  Top-k and ranks over classes: sda_retrieval_select on the value matrix with M := C,
 * chunk_cols := pad64(C) = the pitch and unit norms (v / max(1 * 1, 1e-8) is v; -inf forms a valid key and comes last).
 * Both refuse, before any launch: null pointers, n / N, M, C, G < 1, a chunk_cols that is no positive multiple of 64, S not
 * 16-byte aligned, a pitch below C, a scale that is not positive and finite, an unknown mode. */
int sda_retrieval_class_reduce(const float* S, const float* qsq, const float* csq, const int32_t* order, const int32_t* offsets,
                               float* out, float* row_lse, long out_pitch, int n, int M, int C, int chunk_cols, float scale,
                               int mode, void* stream);
int sda_retrieval_pool_rows(const float* V, long v_pitch, const int32_t* rows, const int32_t* group_offsets, float* out,
                            long out_pitch, int N, int G, int C, void* stream);
/* data parallelism: merge of the per-rank row statistics of the loss (all = the all-gathered [world][3][Bg] table of
 * (row max, row sum exp(l - max), positive's logit or 0) over each rank's block of brain columns): lse[i] = log-sum-exp of global
 * speech row i over the columns of ALL ranks, diag[i] = its positive's logit (utils/loss.py:79's two cross-entropies at the
 * global batch) */
int sda_clip_merge_rows(const float* all, int world, int Bg, float* lse, float* diag, void* stream);
int sda_device_count(void);
/* CU partitions (diagnostic / scheduling experiments): a HIP stream whose kernels run only on the CUs set in `mask` (bit i of
 * word i / 32 = CU i in the runtime's numbering; hipExtStreamCreateWithCUMask), and the CU count persistent grids launched
 * from THIS thread should size themselves for (0 = the device's; returns the previous limit).  The stream is created in
 * the calling process and destroyed with sda_stream_destroy. */
int sda_stream_create_cumask(const uint32_t* mask, int nwords, void** stream);
/* A non-blocking HIP stream of the given priority (hipStreamCreateWithPriority; the device's range on gfx950 is -1 = high,
 * 0 = normal, 1 = LOW — PyTorch's stream pool offers only the first two).  Out-of-range priorities are an error. */
int sda_stream_create_priority(int priority, void** stream);
int sda_stream_destroy(void* stream);
int sda_set_cu_limit(int cus);

/* Batched fp32 matrix product on parameter-sized operands with arbitrary element strides (exact-fp32 MFMA):
 *     C[b][i][j] = sum_{k < K} A[b][i][k] * B[b][k][j],    i < M, j < N, b < batch
 * with A[b][i][k] at A + b * a_b + i * a_i + k * a_k (B, C alike).  Nothing needs padding or alignment.  C is written as
 * c_dtype (SDA_F32 / SDA_BF16 / SDA_F16); elements outside [0, M) x [0, N) are not touched.  Replaces the parameter-space
 * products of the composed SubjectBlock (models.py:111-117: W_subj[s] . (W_sb . W_sa | b_sb)) and of its chain rule. */
typedef struct sda_pgemm_args {
  const float* A;
  const float* B;
  void* C;
  int M, N, K, batch;
  long a_i, a_k, a_b;
  long b_k, b_j, b_b;
  long c_i, c_j, c_b;
  int c_dtype;
} sda_pgemm_args;
int sda_param_gemm(const sda_pgemm_args* a, void* stream);
/* dst[i * d0 + j * d1 + k * d2] = src[i * s0 + j * s1 + k * s2] for (i, j, k) < (n0, n1, n2): fp32, element strides */
int sda_copy3d(float* dst, long d0, long d1, long d2, const float* src, long s0, long s1, long s2, int n0, int n1, int n2,
               void* stream);
/* Asynchronous upload of a small host table (nwords 32-bit words) carried in kernel arguments: no memcpy, no
 * host<->stream synchronisation. The host buffer is read before the call returns. */
int sda_upload_words(void* dst, const void* src_host, long nwords, void* stream);

/* Batch collate (gwilliams2022.py:651-661): per (sample, channel) row of T fp32 samples: subtract the mean of
 * the first baseline_len samples (preproc_utils.py:128-142), RobustScaler over time (median / inter-quartile
 * range, sklearn semantics; preproc_utils.py:69-90), clamp to +-clamp_lim when `clamp`.  rows = B*C, T <= 1024. */
int sda_collate_rows(const float* src, float* dst, long rows, int T, int baseline_len, float clamp_lim, int clamp,
                     void* stream);
/* Same, fused with the segment gather of gwilliams2022.py:129-142: sample b is the window
 * X_session[:, onset : onset + T] of a session recording resident in HBM — win_ptr[b] points at channel 0 of the
 * window, win_cstride[b] is that session's channel stride in elements (device arrays of length B). dst (B, C, T). */
int sda_collate_windows(const float* const* win_ptr, const long* win_cstride, float* dst, int B, int C, int T,
                        int baseline_len, float clamp_lim, int clamp, void* stream);

/* ---- Brennan2018's input path (brennan2018.py:72-152): scale and clamp over the WHOLE recording first, then segment, then
 * baseline-correct each segment.  A "row" of the next two entry points is n_chunks pieces of chunk_len floats, chunk_stride
 * elements apart, starting at x + row * row_stride:
 *     subject-wise (brennan2018.py:114-126) on X (S, C, L): rows = S * C, row_stride = L, n_chunks = 1;
 *     pooled       (brennan2018.py:127-134):                rows = C, row_stride = L, n_chunks = S, chunk_stride = C * L. ---- */
/* RobustScaler.fit over each row (brennan2018.py:117,130): centre[row] = median, scale[row] = 75th - 25th percentile, a zero
 * scale becomes 1 (sklearn).  numpy's "linear" rule: position q * (N - 1) and its fraction in double, the two elements at
 * floor and floor + 1 SELECTED exactly (radix select on order-preserving keys: they are elements of the row), one fp32
 * a + (b - a) * g.  Deterministic: the same input gives the same bits.  2 <= N = n_chunks * chunk_len < 2^31, rows <= 65535.
 * Preconditions: no NaN in the rows; +-inf order like any value (-0.0 counts as +0.0).  scratch: device memory of
 * sda_robust_stats_scratch_bytes(rows) bytes, contents irrelevant before and after. */
long sda_robust_stats_scratch_bytes(long rows);
int sda_robust_stats(const float* x, long rows, long row_stride, int n_chunks, long chunk_len, long chunk_stride,
                     float* centre, float* scale, void* scratch, long scratch_bytes, void* stream);
/* RobustScaler.transform + clamp_ (brennan2018.py:120-124,130-133): y = (x - centre[row]) / scale[row], limited to
 * +-clamp_lim when `clamp`; y is laid out like x (same strides); y == x (in place) is allowed. */
int sda_scale_clamp_rows(const float* x, float* y, long rows, long row_stride, int n_chunks, long chunk_len, long chunk_stride,
                         const float* centre, const float* scale, float clamp_lim, int clamp, void* stream);
/* Segment gather + baseline_correction (brennan2018.py:136-152): dst[b, c, :] = w - mean(w[:baseline_len]) with w the T
 * samples at win_ptr[b] + c * win_cstride[b] (the pointer tables of sda_collate_windows); dst fp32 (B, C, T), any T >= 1;
 * baseline_len = 0 copies the window.  The baseline sum runs in a fixed order. */
int sda_gather_baseline_windows(const float* const* win_ptr, const long* win_cstride, float* dst, int B, int C, int T,
                                int baseline_len, void* stream);

/* ---- Frozen wav2vec 2.0 speech embedder (utils/wav2vec_util.py:14-32 calls the third-party HF Wav2Vec2Model; this is that
 * model's published forward: the layer-norm / stable-layer-norm variant xlsr-53 uses and the group-norm / post-LN variant
 * of wav2vec2-base and -large; the host schedule in speech_decoding_amd/wav2vec2.py chooses).  Every Linear, strided Conv1d and
 * the grouped positional conv run on sda_conv_gemm (kernel size 1 on overlapping-row views); these are the other stages.
 * Activations are row-layout buffers of ONE chunk: row SDA_ROW_PAD + t = frame t. ---- */
/* Feature-encoder layer 0: y = GELU(LayerNorm_C(Conv1d(1 -> C, K, stride)(wave) + bias)); wave fp32 [n_samples] on the
 * device, w fp32 [C][K], T = (n_samples - K) / stride + 1 frames */
int sda_w2v_conv0(const float* wave, long n_samples, const float* w, const float* bias, const float* gamma,
                  const float* beta, void* y, int T, int C, int Cp, int K, int stride, float eps, int dtype, void* stream);
/* Feature-encoder layer 0 of the group-norm checkpoints (feat_extract_norm = "group": wav2vec2-base, -large, -960h):
 *     x[t][c] = Conv1d(1 -> C, K, stride)(wave) (+ bias when not NULL), fp32, never stored
 *     y[SDA_ROW_PAD + t][c] = GELU(gamma[c] * (x[t][c] - mean_c) * rsqrt(var_c + eps) + beta[c]),  pad channels zero
 * mean_c and the biased variance var_c run over ALL T frames of the call.  Two calls on one stream:
 * sda_w2v_conv0_stats leaves stats = scratch[0 .. 3C): shift[C] = x[0][c], the mean of x - shift [C] (so mean_c = shift +
 * that: two numbers, because one fp32 number cannot hold a mean of 1e4 to 1e-7 of a spread of 5), then rsqrt(var + eps)[C];
 * sda_w2v_conv0_groupnorm reads them and computes the conv again (the same arithmetic: the same bits).  The statistics come
 * from the unrounded fp32 conv outputs less the shift: per workgroup (a slice of max(SDA_W2V_GN_SLICE_MIN, ceil(T / SDA_W2V_GN_MAX_WG)) consecutive frames) and wave
 * (every fourth frame of the slice) a Welford mean / sum of centred squares, merged in wave order, then in workgroup order,
 * by Chan's formula.  No atomics, one summation order: the same input gives the same bits, eagerly or from a graph.
 * scratch: sda_w2v_conv0_stats_floats(T, C) floats of device memory (contents irrelevant before); nothing is allocated and
 * the host never waits.  wave fp32 [n_samples] on the device, w fp32 [C][K], T = (n_samples - K) / stride + 1 frames,
 * C <= 1024, max(K, 8) * 64 * ceil(C / 64) * 4 bytes <= 64 KiB; offsets are 64-bit (T up to INT_MAX). */
#define SDA_W2V_GN_SLICE_MIN 256
#define SDA_W2V_GN_MAX_WG 1024
long sda_w2v_conv0_stats_floats(int T, int C);
int sda_w2v_conv0_stats(const float* wave, long n_samples, const float* w, const float* bias, float* scratch,
                        long scratch_floats, int T, int C, int K, int stride, float eps, void* stream);
int sda_w2v_conv0_groupnorm(const float* wave, long n_samples, const float* w, const float* bias, const float* gamma,
                            const float* beta, const float* stats, void* y, int T, int C, int Cp, int K, int stride, int dtype,
                            void* stream);
/* y = LayerNorm over the C valid channels of each of T rows (biased variance, eps inside the root), affine, then GELU
 * when `gelu`; pad channels of y are written as zero.  Cp * sizeof(element) <= 4096 */
int sda_layernorm_rows(const void* x, void* y, const float* gamma, const float* beta, int T, int C, int Cp, float eps,
                       int gelu, int dtype, void* stream);
/* Grouped positional conv, input side: channels [g*gw, (g+1)*gw) of frame t -> xg[g][lead + t][0..gw) (G buffers of
 * group_rows rows x gwp channels; rows outside [lead, lead + T) and channels >= gw must already be zero) */
int sda_w2v_group_split(const void* h, void* xg, int T, int Hp, int gw, int gwp, int G, long group_rows, int lead,
                        int dtype, void* stream);
/* ... output side: out[t][g*gw + c] = h[t][g*gw + c] + f(yg[g][SDA_ROW_PAD + t][c] + bias[g*gw + c]), f = GELU when `gelu`
 * (bias fp32 [G*gw] or NULL).  The G per-group GEMMs between the two are ONE sda_conv_gemm launch: the groups are its
 * "samples" (B = G, sample stride group_rows, widx = 0..G-1 selects the group's weights) */
int sda_w2v_group_merge_add(const void* h, const void* yg, void* out, int T, int Hp, int gw, int gwp, int G, long yg_rows,
                            const float* bias, int gelu, int dtype, void* stream);
/* out = softmax(q k^T * scale) v per head (no mask): q, k row layout with pitch qk_pitch, head h in columns
 * [64h, 64h+64); vt = V transposed, plain matrix [heads*64][vt_pitch >= T rounded up to 64] (columns >= T finite);
 * out row layout with pitch out_pitch.  head_dim must be 64 */
int sda_w2v_attention(const void* q, const void* k, const void* vt, void* out, int T, int heads, int head_dim,
                      long qk_pitch, long vt_pitch, long out_pitch, float scale, int dtype, void* stream);
/* Epilogue of a split-K sda_conv_gemm (partial = its raw fp32 slabs [ksplit][T][Cp], B = 1): y[SDA_ROW_PAD + t][c] =
 * f(sum_s partial[s][t][c] + bias[c]) + res[SDA_ROW_PAD + t][c]; bias / res may be NULL, f = GELU when `gelu` */
int sda_splitk_epilogue(const float* partial, int ksplit, const float* bias, const void* res, void* y, int T, int Cp,
                        int gelu, int dtype, void* stream);
/* out fp32 dense [T][C] = mean of four row-layout hidden states (wav2vec_util.py:18-20) */
int sda_w2v_mean4(const void* a, const void* b, const void* c, const void* d, float* out, int T, int C, int Cp,
                  int dtype, void* stream);

/* ---- MSELoss (speech_decoding/utils/loss.py:15-25): loss = sum_{b,f,t} (y - z)^2 / b_div.  Each operand is described by
 * (pointer, cp, dtype): cp > 0 = a row-layout buffer of cp channels (a multiple of SDA_CH_ALIGN, >= F; both operands the same cp
 * when both are row layout), cp = 0 = a plain contiguous (B, F, T) tensor.  Row-layout buffers 16-byte aligned.  Accumulation in
 * fp32 per element run, fp64 across runs, a fixed reduction order: the same bits every call. ---- */
#define SDA_MSE_PARTIALS 2048
/* loss[0] fp32 = the sum / b_div (b_div: the batch size the mean divides by, the GLOBAL batch under data parallelism);
 * scratch holds SDA_MSE_PARTIALS doubles */
int sda_mse_forward(const void* z, int z_cp, int z_dtype, const void* y, int y_cp, int y_dtype, int B, int F, int T, int b_div,
                    double* scratch, float* loss, void* stream);
/* dz = 2 * (dloss[0] / b_div) * (z - y) in z's form and dtype, dy = -that in y's form and dtype (either may be NULL, not both;
 * dloss is read on the device).  Row-layout outputs get every valid row, pad channels as zeros; their pad rows and slack are not
 * touched (sda_zero_pad_rows) */
int sda_mse_backward(const void* z, int z_cp, int z_dtype, const void* y, int y_cp, int y_dtype, int B, int F, int T, int b_div,
                     const float* dloss, void* dz, void* dy, void* stream);

/* The encoder's gradient with respect to its input (ABI 4): for c < C, t < T
 *     out[b][c][t] = sum_{d < Kp} W[w_b][d][c] * G[b * (T + SDA_ROW_PAD) + SDA_ROW_PAD + t][d],   w_b = widx ? widx[b] : 0
 * G: row-layout data gradient at the output of the SubjectBlock's first linear map, `dtype`, row pitch g_pitch elements
 * (>= Kp, 16-byte rows); W: the (nW, Kp, Cp) matrix the forward applied, `dtype`, contracted over its ROW index (read as a
 * transposed MFMA operand: no transposed copy); Kp % 32 == 0, Cp % 64 == 0, C <= Cp; widx: B device ints in [0, nW), required
 * when nW > 1.  out: a contiguous (B, C, T) tensor of out_dtype (fp32 / bf16 / fp16), fp32 accumulation, every element written
 * once: no zero fill and no row-layout intermediate.  W's bias column (C) and pad columns are never read into the output.
 * Null pointers, bad sizes or misaligned operands return -1 (sda_last_error) and launch nothing. */
int sda_input_grad(const void* G, long g_pitch, const void* W, const int* widx, int nW, int Kp, int Cp, int B, int C, int T,
                   int dtype, void* out, int out_dtype, void* stream);

/* ---- Signal conditioning in front of the data (ABI 4, addition): the FIR band-pass of the raw recordings
 * (mne.filter.filter_data, gwilliams2022.py:253 / brennan2018.py:263) and the polyphase sinc resampler of the audio
 * (torchaudio.functional.resample, gwilliams2022.py:349 / brennan2018.py:172) are both a fixed matrix applied to strided
 * windows of each row (csrc/window_gemm.hip):
 *     out[r][m * N + j] = sum_{k < K} x[r][m * S + k] * B[k][j],     r < rows, m < frames, j < N
 * fp32 in and out, exact-fp32 MFMA (a k-ordered fmaf chain per output).  x: rows x_row_stride elements apart, of which
 * x[r][0 ... (frames - 1) * S + K - 1] must be readable — nothing else is read; B: K x N row-major; out: rows out_row_stride
 * elements apart, out[r][0 ... frames * N - 1] written and nothing else.  Any rows, frames, S, K, N >= 1; no padding or
 * alignment of N, K or the pointers beyond the element's.  Null pointers, non-positive sizes, out_row_stride < frames * N and
 * x_row_stride < (frames - 1) * S + K return -1 (sda_last_error) and launch nothing. */
int sda_window_gemm_f32(const float* x, long x_row_stride, int rows, long frames, int S, int K, const float* B, int N,
                        float* out, long out_row_stride, void* stream);

/* ---- Log-mel speech features (ABI 4, addition): the pass behind the STFT (csrc/mel_power.hip).  The STFT is
 * sda_window_gemm_f32 with S = hop, K = n_fft, N = 2 * n_freqs and B = window x DFT, real and imaginary parts interleaved;
 * its output is this entry's `spec` as it stands (torchaudio.transforms.MelSpectrogram(power=2.0), then log(eps + mel)):
 *     P[r][m][b]   = spec[r][m * spec_pitch + 2 b]^2 + spec[r][m * spec_pitch + 2 b + 1]^2,        b < n_freqs
 *     mel[r][j][m] = sum_{b < n_freqs} P[r][m][b] * fb[b * n_mels + j],                            j < n_mels, m < frames
 *     out[r][j * out_pitch + m] = log_eps < 0 ? mel : logf(log_eps + mel),                         r < rows
 * fp32 in and out; P = fmaf(im, im, re * re); exact-fp32 MFMA (one fmaf chain per output in increasing b).  spec: rows
 * spec_row_stride elements apart, frame m at m * spec_pitch, spec_pitch >= 2 * n_freqs; only the 2 * n_freqs floats of each of
 * the `frames` frames are read.  fb: n_freqs x n_mels row-major.  out: rows out_row_stride elements apart, each
 * (n_mels, out_pitch) with out_pitch >= frames: out[r][j][0 ... frames - 1] written and nothing else (features x frames, the
 * layout of the speech tables).  Any rows, frames, n_freqs, n_mels >= 1; no alignment beyond the element's.  No atomics: the
 * same bits on every call.  Null pointers, non-positive sizes, spec_pitch < 2 * n_freqs, out_pitch < frames,
 * spec_row_stride < (frames - 1) * spec_pitch + 2 * n_freqs and out_row_stride < (n_mels - 1) * out_pitch + frames return -1
 * (sda_last_error) and launch nothing. */
int sda_mel_power_f32(const float* spec, long spec_row_stride, long spec_pitch, int rows, long frames, int n_freqs,
                      const float* fb, int n_mels, float log_eps, float* out, long out_row_stride, long out_pitch, void* stream);

/* ---- The STFT as a power-of-two FFT (ABI 4, addition): the alternative to sda_window_gemm_f32 with the window x DFT matrix
 * (csrc/stft_fft.hip), for r < rows, m < frames, b < n_freqs = n_fft / 2 + 1
 *     X[r][m][b] = sum_{k < n_fft} window[k] * x[r][m * hop + k] * exp(-2 pi i b k / n_fft)
 *     out[r][m * out_pitch + 2 b] = Re X[r][m][b],     out[r][m * out_pitch + 2 b + 1] = Im X[r][m][b]
 * fp32 in and out: a half-size complex transform of z[k] = y[2 k] + i y[2 k + 1], y = window * x (Stockham radix-4 passes, one
 * radix-2 pass when log2(n_fft / 2) is odd), then the real-FFT split step.  x: rows x_row_stride elements apart, of which
 * x[r][0 ... (frames - 1) * hop + n_fft - 1] is read and nothing else.  window: n_fft floats (normalisation and any zero padding
 * of a shorter window folded in by the caller).  twiddle: n_fft / 2 pairs (cos(2 pi j / n_fft), -sin(2 pi j / n_fft)), j < n_fft / 2.
 * out: rows out_row_stride elements apart, frame m at m * out_pitch; exactly the 2 * n_freqs floats of each frame are written
 * (with out_pitch = 2 * n_freqs: the layout the window GEMM leaves and sda_mel_power_f32 reads); the imaginary parts of bin 0
 * and of the Nyquist bin are exact zeros.  n_fft a power of two, 32 <= n_fft <= 2048; any hop, rows, frames >= 1; no alignment
 * beyond the element's.  No atomics: the same bits on every call.  Null pointers, non-positive sizes, an unsupported n_fft,
 * out_pitch < 2 * n_freqs, out_row_stride < (frames - 1) * out_pitch + 2 * n_freqs and x_row_stride < (frames - 1) * hop + n_fft
 * return -1 (sda_last_error) and launch nothing. */
int sda_stft_fft_f32(const float* x, long x_row_stride, int rows, long frames, int hop, int n_fft, const float* window,
                     const float* twiddle, float* out, long out_row_stride, long out_pitch, void* stream);

/* ---- Gradient guard (ABI 4, addition): global-norm clipping and the fp16 overflow guard decided on the device, three launches
 * over the descriptor table sda_adam_multi takes (csrc/grad_guard.hip, csrc/param_ops.hip).  No host read-back anywhere: the
 * decision lives in `state`, SDA_GUARD_STATE doubles on the device, at the slot indices below.
 *   SCALE     the loss scale the NEXT backward is multiplied by (set by the caller before the first step, >= 1)
 *   SKIP      1 when the last finish found a non-finite gradient (the guarded Adam then writes nothing), else 0
 *   STEP      number of APPLIED steps (the bias corrections' exponent)     GOOD     applied steps since the last skip or growth
 *   SKIPPED   number of skipped steps                                      NORM     last unscaled gradient norm (+inf on a skip)
 *   COEF      last factor on the stored gradients: (1 / scale used) x clip factor (0 on a skip)
 *   BC1, BC2_SQRT   1 - beta1^STEP and sqrt(1 - beta2^STEP), rounded to float, as sda_adam_multi's host code computes them
 *   NONFINITE last count of inf / NaN gradient elements                    SUMSQ    last sum of squares of the finite ones */
#define SDA_GUARD_SCALE 0
#define SDA_GUARD_SKIP 1
#define SDA_GUARD_STEP 2
#define SDA_GUARD_GOOD 3
#define SDA_GUARD_SKIPPED 4
#define SDA_GUARD_NORM 5
#define SDA_GUARD_COEF 6
#define SDA_GUARD_BC1 7
#define SDA_GUARD_BC2_SQRT 8
#define SDA_GUARD_NONFINITE 9
#define SDA_GUARD_SUMSQ 10
#define SDA_GUARD_STATE 16
/* doubles sda_grad_sumsq_multi writes for n tensors of at most max_n elements: 2 * n * gx, gx = min(ceil(max_n / 1024), 256)
 * (sda_adam_multi's grid rule); -1 for n < 1 or max_n < 1 */
long sda_grad_guard_parts(int n, long max_n);
/* partials[t][b][0] = sum of g^2 over the FINITE gradient elements workgroup b of tensor t reads (the elements
 * sda_adam_multi's workgroup b updates), every product and every add in double; partials[t][b][1] = how many of them are inf or
 * NaN.  Dense [n][gx][2]; every slot is written, zeros by a workgroup past its tensor's end.  Only descs[t].grad, n and aligned
 * are read.  Fixed summation order (a thread's elements in index order, then a fixed tree over the 256 threads): the same bits
 * on every call. */
int sda_grad_sumsq_multi(const sda_adam_desc* descs, int n, long max_n, double* partials, void* stream);
/* One workgroup: sums the n * gx slots (thread t adds slots t, t + 256, ... in index order, then the fixed tree) and takes the
 * decision in double.  scale = state[SCALE], norm = sqrt(sum) / scale.
 *   count > 0:  SKIP = 1, SKIPPED += 1, GOOD = 0, STEP stays, COEF = 0, NORM = +inf, and with dynamic != 0 SCALE = max(1, SCALE / 2).
 *   otherwise:  SKIP = 0, STEP += 1, GOOD += 1; with dynamic != 0 and GOOD >= growth_interval, SCALE = min(max_scale, 2 SCALE) and
 *               GOOD = 0; COEF = (1 / scale) * min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_'s rule; max_norm <= 0
 *               or +inf: the clip factor is exactly 1); BC1 / BC2_SQRT from the new STEP and the float betas.
 * Null pointers, n < 1, gx < 1, growth_interval < 0, a NaN max_norm and max_scale < 1 return -1 (sda_last_error), no launch. */
int sda_grad_guard_finish(const double* partials, int n, int gx, double* state, double max_norm, float beta1, float beta2,
                          long growth_interval, double max_scale, int dynamic, void* stream);
/* sda_adam_multi behind the guard: nothing is written when state[SKIP] is set; otherwise the update of sda_adam_multi on
 * fl32(grad * (float)state[COEF]) with the bias corrections read from state.  The stored gradients are not modified. */
int sda_adam_multi_guarded(const sda_adam_desc* descs, int n, long max_n, float lr, float beta1, float beta2, float eps,
                           const double* state, void* stream);

/* ---- Lag products of a time-lagged ridge regression (ABI 4, addition): the normal equations of the backward mTRF, the linear
 * decoding baseline (mne.decoding.TimeDelayingRidge, edge_correction=False), csrc/lagged_cov.hip:
 *     out[s][d][i][j] = sum_{r in row slice s} a[r + d][i] * b[r][j],     d < L, i < Ap, j < Bp
 * fp32 in and out, exact-fp32 MFMA (per output a k-ordered fmaf chain over the slice's rows).  Lag layout: a and b are `rows` rows
 * of a_pitch / b_pitch floats, channels-last, of which the first Ap / Bp are read (the channel counts padded to 64, pad channels
 * zero); sample n of a (B, C, T) tensor owns rows n (T + H) ... n (T + H) + T - 1 and H >= L - 1 zero rows follow it, so a lagged
 * row that leaves its sample reads zeros and nothing is masked per sample.  rows = B (T + H).  Rows >= rows are never read and count
 * as zero.  a = b gives the Gram blocks A_d, a = x, b = y the cross products R_l.  The rows are cut into
 * sda_lagged_cov_slices(rows, L, Ap, Bp) slices, a number that depends on these four alone; slice s writes every element of slab s
 * of out = [slices][L][Ap][Bp] (sda_lagged_cov_scratch_floats floats) and the caller sums the slabs in fixed order
 * (sda_reduce_slabs, or in double).  No atomics: the same bits on every call.  Null pointers, non-positive sizes, Ap or Bp not a
 * multiple of 64, a pitch smaller than its width or not a multiple of 4, operands not 16-byte aligned and L - 1 > H return -1
 * (sda_last_error) and launch nothing; the two size functions return -1 the same way. */
int sda_lagged_cov_slices(long rows, int L, int Ap, int Bp);
long sda_lagged_cov_scratch_floats(long rows, int L, int Ap, int Bp);
int sda_lagged_cov_f32(const float* a, long a_pitch, const float* b, long b_pitch, long rows, int L, int H, int Ap, int Bp,
                       float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_AMD_H */
