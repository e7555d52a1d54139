/*
 * ls_hip.h -- C-ABI of the MI355X (gfx950) kernel library libls_hip.so for the
 * LatentSync inference denoising hot path.
 *
 * The reference has no FFI on this path: its swap points are
 * the duck-typed Python objects injected into LipsyncPipeline.__init__
 * (latentsync/pipelines/lipsync_pipeline.py:49-124).  This library sits UNDER
 * those objects; the host package latentsync_amd binds it with ctypes.  Every
 * entry point below names the reference interface whose arithmetic it replaces.
 *
 * Conventions
 *   - All tensors are caller-allocated device buffers (plain pointers); no entry
 *     point allocates, frees or synchronises, so every call can be captured into
 *     a hipGraph.  `stream` is a hipStream_t (NULL = default stream).
 *   - Activations are "pixel-major" (NHWC): frames are folded into the image
 *     index exactly like InflatedConv3d's "b c f h w -> (b f) c h w"
 *     (latentsync/models/resnet.py:10-18); element (img, y, x, c) lives at
 *     ((img*H + y)*W + x)*ld + c.  Storage type is bf16 (uint16_t bit pattern)
 *     unless a field says fp32.
 *   - Return value: 0 = LS_OK, otherwise an ls_status; ls_last_error() returns
 *     a thread-local message for the last failure.
 */
#ifndef LS_HIP_H
#define LS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LS_ABI_VERSION 14

typedef enum {
  LS_OK = 0,
  LS_ERR_INVALID = 1,  /* bad shape / alignment / unsupported combination */
  LS_ERR_LAUNCH = 2,   /* hipLaunchKernel / hipGetLastError failure       */
  LS_ERR_WORKSPACE = 3 /* workspace missing or too small                   */
} ls_status;

enum { LS_ACT_NONE = 0, LS_ACT_GEGLU = 1, LS_ACT_GELU = 2, LS_ACT_SILU = 3 };

/*
 * Fused implicit-GEMM convolution / linear layer on bf16 MFMA
 * (v_mfma_f32_16x16x32_bf16), fp32 accumulate.
 *
 *   Y[m, n] = epilogue( sum_k A[m, k] * Wp[n, k] )
 *
 * A is never materialised: row m is an output pixel (img, yo, xo); column
 * k reads input channel ci of the tap's source pixel -- k = tap*Cin + ci, or for
 * ksize 3 with Cin % 64 == 0 (ABI 10) k = (ci/64)*576 + tap*64 + ci%64 -- from x1
 * (ci < C1) or x2 (ci >= C1, the fused torch.cat of the up blocks,
 * unet_blocks.py:624,745).  Optional prologue per element (fused GroupNorm
 * apply + SiLU of ResnetBlock3D, resnet.py:185-186 / 207-213):
 *   a = x * aff_scale[s, ci] + aff_shift[s, ci]; if (silu_in) a = silu(a)
 * with s = img / imgs_per_sample.  Zero padding is applied after the prologue.
 * ksize 1 = linear / 1x1 conv (Transformer proj_in/out, q/k/v/out, FF, shortcut);
 * ksize 3 = InflatedConv3d 3x3 (conv1/2, conv_in/out, samplers).
 * stride 2 + pad 1 = Downsample3D (resnet.py:89), stride 2 + pad 0 = the SD-VAE
 * downsampler after F.pad(0,1,0,1); upsample = nearest x2 fused into the
 * gather (Upsample3D, resnet.py:53-73).
 * upsample = 1: Wp is the ordinary 9-tap 3x3 operand.  upsample = 2: the same layer with
 * PHASE-PACKED weights.  The 2 x 2 output pixels of an input pixel read one 3 x 3 input
 * neighbourhood, and the three row taps of output parity py land on two input rows
 * (py = 0: rows y-1, y with weights w[0], w[1]+w[2]; py = 1: rows y, y+1 with weights
 * w[0]+w[1], w[2]; the same in x), so the layer is four 2x2 convs over the input image, one
 * per parity ph = 2 py + px, 4/9 of the multiply-adds.  Wp is then [4][N][K], K = 4*Cin,
 * k = (ci / 64) * 256 + (2 dy + dx) * 64 + ci % 64 (latentsync_amd/packing.py,
 * pack_phase_weight: taps summed in fp32, rounded once).  It needs ksize 3, Cin % 64 == 0,
 * stride 1, pad 1, Ho x Wo = 2H x 2W and no affine prologue (else LS_ERR_INVALID).  It runs
 * on the halo-tile kernel (ls_conv_path 4: H and W multiples of 16, N % 160 or % 128 == 0,
 * 16 < N <= 640, one source) or else on the tiled kernels (ls_conv_path 5: per parity a pad-1
 * conv in input space over 4 of the 9 tap positions, the parity a grid slice; one source, no
 * rowvec, no activation, bf16 output, N % 8 == 0, ldy % 8 == 0, no split-K; gn_colsum_out by a
 * read pass).  ls_conv_path answers -1 elsewhere (ls_conv2d then fails with LS_ERR_INVALID:
 * callers keep upsample = 1 for those shapes).
 *
 * Wp is the packed weight [N][K]: K = ksize*ksize*Cin rounded up to 64, in the same
 * k order: tap-major, except ksize 3 with Cin % 64 == 0, which is channel-chunk-major
 * (the 9 taps of a 64-channel chunk consecutive; see latentsync_amd/packing.py).
 * Epilogue, in this order:
 *   if (ln_rowstats)  acc = rstd[m] * (acc - mean[m] * ln_colsum[n])
 *       -- LayerNorm of the A rows folded into the GEMM: with Wp = W * gamma
 *       (per input column), bias = b + W beta and ln_colsum[n] = sum_k Wp[n, k],
 *       this equals W LN(x) + b exactly in real arithmetic (BasicTransformerBlock
 *       norm1/2/3 -> to_q|k|v / to_q / ff.net.0, attention.py:145-199;
 *       TemporalTransformerBlock norms -> q|k|v / FF, motion_module.py:240-313);
 *       ln_rowstats = (mean, rstd) fp32 pairs per row from ls_row_stats
 *   v = acc + bias[n] + rowvec[((m / rows_per_vec) % rowvec_mod) * rowvec_ld + n]
 *       (temb add, resnet.py:190-205; W pe of the motion positional encoding;
 *        rowvec_mod 0 = no modulo)
 *   v = (v + res[m, n]) * out_scale                      (residual, resnet.py:221)
 *   act: GEGLU pairs packed columns (32b+i, 32b+16+i) -> out col 16b+i,
 *        out = h * gelu_erf(g) (diffusers GEGLU), N % 32 == 0, bias only: GEGLU with a
 *        rowvec, a residual or an out_scale other than 1 is LS_ERR_INVALID;
 *        GELU (whisper MLP); SiLU.
 * N, ldy and ldr need not be multiples of 8: when N % 8, ldy % 8 or (with a residual)
 * ldr % 8 is non-zero, the tiled kernels store element by element instead of 16 bytes at
 * a time (bias, rowvec, residual and output are then only read / written below column N).
 * C1, C2, ld1 and ld2 must be multiples of 8 (LS_ERR_INVALID otherwise).
 * split_k > 1 needs `workspace` of split_k*M*N fp32 (ls_conv_workspace_bytes).
 */
typedef struct {
  const uint16_t* x1; const uint16_t* x2;
  int32_t C1, C2;            /* channels read from x1 / x2 (C2 = 0: no concat) */
  int32_t ld1, ld2;          /* pixel pitch (elements) of x1 / x2             */
  int32_t n_img, H, W;       /* input images / resolution (ksize 1: H=1, W=rows) */
  int32_t Ho, Wo;            /* output resolution                              */
  int32_t ksize, stride, pad, upsample;
  const float* aff_scale; const float* aff_shift; int32_t imgs_per_sample; int32_t silu_in;
  const uint16_t* w; int32_t K; int32_t N;
  const float* bias;
  const float* rowvec; int32_t rows_per_vec; int32_t rowvec_ld; /* rowvec_ld 0 = N */
  const uint16_t* res; int32_t ldr; float out_scale;
  int32_t act;
  void* y; int32_t ldy; int32_t y_f32;
  int32_t split_k;           /* 0 = choose automatically                       */
  void* workspace; size_t workspace_bytes;
  const float* ln_rowstats;  /* NULL or (mean, rstd) per A row (ksize 1 only)  */
  const float* ln_colsum;    /* [N] column sums of Wp (with ln_rowstats)       */
  int32_t rowvec_mod;        /* 0 = none                                       */
  float* row_stats_out;      /* NULL or fp32 [M][2] (mean, rstd) of each output row (ksize 1,
                                LayerNorm statistics for the next folded GEMM; the row-block
                                kernel emits them from its epilogue, other paths run
                                ls_row_stats on y)                                  */
  float row_stats_eps;       /* LayerNorm eps of row_stats_out (0 = 1e-5)        */
  float* gn_colsum_out;      /* NULL or fp32 [M / LS_GN_SLOT_ROWS][2][N]: per 128-row slot and
                                output column, the sum and the sum of squares of the stored
                                bf16 values (GroupNorm statistics of y for
                                ls_groupnorm_colsum; M % 128 == 0, bf16 output, no GEGLU).
                                The tiled kernels emit them from their epilogue; the other
                                paths (split-K, row-block, small tiles) read y once more. */
} ls_conv_desc;

#define LS_GN_SLOT_ROWS 128

int ls_conv2d(const ls_conv_desc* d, void* stream);
/* Which kernel family ls_conv2d will launch for d (the family of its plan, see ls_conv_plan:
 * the same decision, taken once, not a separate walk): 0 = tiled DMA GEMM, 1 = row-block
 * GEMM (K = 320 / 640 linears; also takes the GroupNorm affine prologue on its
 * register-resident A rows), 2 = register-staged tiled GEMM (affine prologue
 * elsewhere -- callers materialise the affine with ls_groupnorm_apply instead),
 * 3 = halo-tile 3x3 conv (ABI 12: 3x3 / stride 1 / pad 1 (or a nearest-x2 upsample without an
 * input affine, round 6), Cin % 64 == 0, W in {16, 32,
 * 64} or a multiple of 64, N % 160 or % 128 == 0; takes the GroupNorm affine + SiLU on
 * its input, once per pixel, and the dual-source concat), 4 = the halo-tile kernel's phase
 * form (upsample = 2), 5 = the tiled kernels' phase form (upsample = 2), -1 = invalid
 * descriptor or upsample = 2 with no phase-form kernel.
 * Host-only, no launch. */
int ls_conv_path(const ls_conv_desc* d);
size_t ls_conv_workspace_bytes(const ls_conv_desc* d);

/* The plan of an ls_conv2d call: the one kernel instance it launches, with its geometry, and
 * the passes that follow it.  ls_conv2d makes this plan and runs it; ls_conv_path is its
 * `family`, ls_conv_workspace_bytes its `workspace_bytes`.  The order of the decision:
 *   1. upsample = 2: the halo-tile kernel's phase form (4), else the tiled one (5), else an error;
 *   2. the halo-tile 3x3 conv (3);
 *   3. the row-block GEMM (1) with row_stats_out and gn_colsum_out in its epilogue;
 *   4. the row-block GEMM with row_stats_out, gn_colsum_out by a read pass over y;
 *   5. with row_stats_out and no such instance: the row-block GEMM without the statistics
 *      (gn_colsum_out in the epilogue, else by the read pass), ls_row_stats over y at the end;
 *   6. the tiled kernels (0; 2 with an affine prologue or tuning key 1): gn_colsum_out in the
 *      epilogue where the tile has it, else by the read pass; ls_row_stats over y at the end.
 * A split-K the workspace of d cannot hold is reduced to what fits before 1. (a NULL workspace
 * is never split automatically).  Fields that do not apply to the family are -1.
 * Within 6., a 3x3 / stride 1 / pad 1 conv with Cin % 64 == 0, no affine prologue and no split-K
 * runs the 256-row tiles position-major (`posmajor`; tuning key 22) where that costs fewer
 * tap-units: a tile is 256 frames at one pixel, and the taps that fall into the zero padding
 * there are left out of its K loop.  The output is bit-identical to the standard raster's. */
typedef struct {
  int32_t family;                  /* ls_conv_path code                                      */
  int32_t bm, bn, ks, tapu;        /* tiled kernels: tile (bm 256: the 8-wave kernels), gather */
  int32_t buf, epi;                /* LDS-DMA tiled kernels: buffer-descriptor DMA; epilogue
                                      0 plain, 1 GEGLU, 2 general, 3 plain phase form         */
  int32_t split;                   /* split-K slabs (1 = none)                               */
  int32_t rb_kt, rb_fm, rb_flags;  /* row-block GEMM: K / 32, 16-row fragments per wave, flags 1 LN
                                      fold, 2 residual, 4 rowvec, 8 GEGLU, 16 row statistics,
                                      32 GroupNorm column sums, 64 affine prologue           */
  int32_t halo_bn, halo_th, halo_gn, halo_cs, halo_ph; /* halo-tile conv: columns, patch rows,
                                      input affine, column sums, phase form                  */
  int32_t grid, threads, lds_bytes;  /* the launch: blocks, threads per block, dynamic LDS   */
  int32_t reduce;                  /* trailing passes, in this order: the split-K reduce,      */
  int32_t colsum_rows;             /* the gn_colsum_out read pass over this many rows of y (0: none), */
  int32_t row_stats;               /* ls_row_stats over y                                    */
  int64_t workspace_bytes;         /* what the plan's split-K asks for, before it is fitted  */
  int32_t posmajor;                /* tiled kernels: 1 = the position-major form of a 3x3 conv, 0 = the
                                      standard raster (appended last: the offsets above are unchanged) */
} ls_conv_plan_info;
/* Host-only, no launch, no GPU needed. */
int ls_conv_plan(const ls_conv_desc* d, ls_conv_plan_info* out);
/* The launch order of the position-major form: block `block` of the H x W x groups x ntn grid
 * (groups = ceil(n_img / 256) frame groups, ntn column tiles) -> out[0..3] = pixel position
 * y * W + x, frame group, column tile, valid taps (4, 6 or 9).  The kernel runs the same
 * function.  Host-only.  LS_ERR_INVALID: H or W < 3, groups or ntn < 1, block out of range. */
int ls_conv_posmajor_tile(int32_t H, int32_t W, int32_t groups, int32_t ntn, int32_t block, int32_t* out);

/*
 * GroupNorm statistics -> per-(sample, channel) affine for the consumer's
 * prologue.  Replaces nn.GroupNorm of ResnetBlock3D (5-D: stats span all frames
 * of a sample, resnet.py:140,164; unet.py:236), Transformer3DModel.norm and
 * TemporalTransformer3DModel.norm (4-D per frame, attention.py:51,
 * motion_module.py:101) and the SD-VAE GroupNorms.
 * Input: n_samples * pix_per_sample pixels of C = C1 + C2 channels (x2 = concat).
 * Output: scale[s, c] = gamma[c] * rstd[s, g]; shift[s, c] = beta[c] - mean[s, g] * scale.
 * One launch: the last-arriving block of a sample merges the split partials.
 * workspace >= ls_groupnorm_workspace_bytes(); its first 4 KiB are arrival
 * counters that must be zero before the first call (each call re-arms them).
 */
int ls_groupnorm(const uint16_t* x1, const uint16_t* x2, int32_t C1, int32_t C2, int32_t n_samples,
                 int64_t pix_per_sample, int32_t groups, float eps, const float* gamma, const float* beta,
                 float* scale, float* shift, void* workspace, size_t workspace_bytes, void* stream);
size_t ls_groupnorm_workspace_bytes(int32_t n_samples, int32_t groups);

/*
 * GroupNorm statistics from producer column sums (ls_conv_desc.gn_colsum_out or
 * ls_gn_colsum): the same affine as ls_groupnorm without reading the activation
 * again.  cs1 / cs2: [n_samples * pix_per_sample / 128][2][C1 | C2] of x1 / x2;
 * pix_per_sample % LS_GN_SLOT_ROWS == 0.  Slot sums are merged in fp64 per
 * (sample, group); var = E[x^2] - mean^2 (the fp32 slot sums bound the relative
 * variance error by ~1e-7 * (1 + mean^2 / var)).
 */
int ls_groupnorm_colsum(const float* cs1, const float* cs2, int32_t C1, int32_t C2, int32_t n_samples,
                        int64_t pix_per_sample, int32_t groups, float eps, const float* gamma, const float* beta,
                        float* scale, float* shift, void* stream);

/* The column sums of an existing bf16 [M][ldy] tensor (first N columns) by a read
 * pass: out [M / 128][2][N] as ls_conv_desc.gn_colsum_out. */
int ls_gn_colsum(const uint16_t* y, int64_t ldy, int64_t M, int32_t N, float* out, void* stream);

/* Materialised GroupNorm(+SiLU) apply over an optional channel concat
 * (x1 | x2) -> y [n_pix][C1 + C2]: the input of a 3x3 conv, whose gather would
 * otherwise recompute the affine + SiLU once per tap and per N-tile. */
int ls_groupnorm_apply(const uint16_t* x1, const uint16_t* x2, int32_t C1, int32_t C2, int64_t n_pix,
                       int64_t pix_per_sample, const float* scale, const float* shift, int32_t silu, uint16_t* y,
                       void* stream);

/*
 * LayerNorm over the last dim (nn.LayerNorm of BasicTransformerBlock
 * attention.py:145,157,172 and TemporalTransformerBlock motion_module.py:195,201;
 * whisper LayerNorm model.py:29-31).  Optional fused temporal positional
 * encoding add (VersatileAttention pos_encoder, motion_module.py:267-268):
 *   y[r, c] += pe[(r / pe_rows_per_frame) % pe_frames, c]   (pe fp32 [len][C]).
 * x rows are ldx elements apart (ldx >= C, multiple of 8); y is dense [rows][C].
 */
int ls_layernorm(const uint16_t* x, int64_t ldx, int64_t rows, int32_t C, float eps, const float* gamma,
                 const float* beta, const float* pe, int32_t pe_rows_per_frame, int32_t pe_frames, uint16_t* y,
                 void* stream);

/* Per-row LayerNorm statistics (mean, rstd = 1/sqrt(var + eps)) fp32 pairs of
 * x [rows][C] (row pitch ldx): the producer side of the LayerNorm -> linear fold
 * (ls_conv_desc.ln_rowstats). */
int ls_row_stats(const uint16_t* x, int64_t ldx, int64_t rows, int32_t C, float eps, float* stats, void* stream);

/*
 * Multi-head attention softmax(Q K^T * scale) V on MFMA with LDS-staged K/V
 * tiles (F.scaled_dot_product_attention of Attention.forward attention.py:271,
 * VersatileAttention motion_module.py:300, whisper qkv_attention model.py:88-100,
 * SD-VAE mid attention).  Element (b, h, i, d) of T in {q,k,v,o} is at
 *   T + (b / z2)*T_sb1 + (b % z2)*T_sb2 + i*T_si + h*T_sh + d
 * so spatial (rows = tokens), temporal ("(b f) s c -> (b s) f c") and audio
 * cross-attention (Nk = 50) are strided views of the projection outputs.
 * head_dim <= 512.
 */
typedef struct {
  const uint16_t* q; const uint16_t* k; const uint16_t* v; uint16_t* o;
  int64_t q_sb1, q_sb2, q_si, q_sh;
  int64_t k_sb1, k_sb2, k_si, k_sh;
  int64_t v_sb1, v_sb2, v_si, v_sh;
  int64_t o_sb1, o_sb2, o_si, o_sh;
  int32_t batch, z2, heads, nq, nk, head_dim;
  float scale;
} ls_attn_desc;

int ls_attention(const ls_attn_desc* d, void* stream);

/*
 * The same attention with the P V product in fp8 (BASELINE.json configs[4], "fp8 MFMA
 * attention"; replaces the same SDPA call, attention.py:271): QK^T and the softmax as
 * ls_attention (bf16 MFMA, fp32), P and V in OCP e4m3 on the block-scaled MFMA
 * v_mfma_scale_f32_16x16x128_f8f6f4.  V is quantised by a pre-pass into `workspace`
 * with one e8m0 scale per (head dim, 128-key tile) -- block scaling, the tile's max
 * mapped into [128, 256), the same scale for all four 32-key MX blocks of a tile; P (<= 2^8 by the kernel's rescale threshold) uses scale 1 and the
 * row sums come from the same e4m3 P.  Two launches (quantise, attend), capturable.
 * head_dim 40 or 80 (the UNet's 64^2 / 32^2 levels); q/k/v rows 16-B aligned, o rows 8-B aligned
 * (o and every o stride a multiple of 4 elements: the kernel stores 8 bytes at a time).
 * Workspace: ls_attention_fp8_workspace_bytes(d) (0 = unsupported head_dim), 16-B aligned;
 * its layout is documented in ls_attn.hip (the tests read it back).
 */
size_t ls_attention_fp8_workspace_bytes(const ls_attn_desc* d);
int ls_attention_fp8(const ls_attn_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The motion module's temporal self-attention fused with its input side: replaces, per
 * VersatileAttention block (latentsync/models/motion_module.py:203-218 and :262-313),
 *   LayerNorm(h) -> "(b f) s c -> (b s) f c" + pe[:f] -> to_q / to_k / to_v -> SDPA over
 *   the f frames (8 heads) -> "(b s) f c -> (b f) s c"
 * writing the attention output o (before to_out).  The q|k|v projections never reach HBM.
 *   x, o   : (n_samples * F * S) rows of C bf16, row (b*F + f)*S + s, pitches ldx / ldo
 *   gamma  : fp32 [C], the LayerNorm weight;  bpe: fp32 [16][C], LayerNorm bias + pe row f
 *   w      : bf16 [3C][C] packed per 80-column group g and 16-channel tile t = 0..4: q rows
 *            80g+16t..+15 scaled by log2(e)/sqrt(C/8), then the same k rows, then v rows
 *            (latentsync_amd/ops.py pack_temporal)
 * C = 320 (d 40) or 640 (d 80), heads = 8, 1 <= F <= 16, S % 16 == 0 (C = 320) or S % 8 == 0
 * (C = 640), 16-B aligned pointers, pitches % 8 == 0.
 */
typedef struct {
  const uint16_t* x;
  int32_t ldx;
  const float* gamma;
  const float* bpe;
  const uint16_t* w;
  uint16_t* o;
  int32_t ldo;
  int32_t C, heads, n_samples, F, S;
  float eps;
} ls_tattn_desc;

int ls_temporal_attention(const ls_tattn_desc* d, void* stream);

/*
 * FeedForward of a BasicTransformerBlock / TemporalTransformerBlock with its LayerNorm and
 * residual, one launch (ABI 11; diffusers FeedForward(dim, "geglu"), attention.py:174-199
 * norm3 + ff, motion_module.py:240-313 ff_norm + ff):
 *   y = x + W2 (h * gelu_erf(g)) + b2,  [h | g] = W1 LN(x) + b1
 * x, y: bf16 rows [M][ldx] / [M][ldy]; ln_rowstats: (mean, rstd) fp32 pairs of the x rows
 * (the producing GEMM's row_stats_out); w1: bf16 [2*inner][C], the GEGLU rows interleaved
 * in 16-row blocks (packing.geglu_interleave) with LayerNorm gamma folded in (W1 * gamma),
 * b1: fp32 [2*inner] = b1 + W1 beta in the same order; w2: bf16 W2 [C][inner] re-packed
 * per 32-column chunk (packing.pack_ff_w2: [inner/32][C][32], columns permuted and 16-B
 * pieces swizzled to the kernel's register layout); b2: fp32 [C].  C = 320, inner = 1280
 * (the 32x32 level) only.  The 4C-wide GEGLU intermediate never reaches memory.
 */
typedef struct {
  const void* x;
  const float* ln_rowstats;
  const void* w1;
  const float* b1;
  const void* w2;
  const float* b2;
  void* y;
  int64_t M;
  int32_t ldx, ldy, C, inner;
} ls_ff_desc;

int ls_feedforward(const ls_ff_desc* d, void* stream);

/*
 * The 32x32-level tail of a Transformer3DModel block / motion module in ONE launch (ABI
 * 13): the attention branch's out-projection + residual, the LayerNorm, the GEGLU
 * FeedForward + residual and proj_out + the block input, with the GroupNorm column sums
 * of the result (replaces attention.py:174-199 attn2.to_out + norm3 + ff and :110-118
 * proj_out; motion_module.py:262-313 the last to_out + ff_norm + ff and :126-151 proj_out):
 *   h2 = o Wo^T + bo + h1,  y = h2 + W2 (h * gelu_erf(g)) + b2 with [h | g] = W1 LN(h2) + b1,
 *   z  = y Wp^T + bp + xb
 * Rows: o, h1, xb, z bf16 [M][ld*] (M % 128 == 0).  LN statistics are computed in the
 * kernel over the bf16-rounded h2 (biased variance, eps).  Weights (packing.pack_ff_chain):
 * wo, wp bf16 [C/32][C][32] k-step images (wp and w1 with each 32-wide k block permuted to
 * the register order of pack_ff_w2, wo in natural order; 16-B pieces swizzled as w2); w1
 * bf16 [2*inner][C] (GEGLU rows interleaved, LN gamma folded), b1 = b1 + W1 beta; w2 as
 * ls_feedforward; bo, b2, bp fp32 [C].  cs_out: NULL or fp32 [M/128][2][C] column sums
 * (Σz, Σz²) of the stored z per 128-row slot (ls_conv_desc.gn_colsum_out's layout).
 * C = 320, inner = 1280 only.  h2 and y never reach memory.
 */
typedef struct {
  const void* o;
  const void* wo;
  const float* bo;
  const void* h1;
  const void* w1;
  const float* b1;
  const void* w2;
  const float* b2;
  const void* wp;
  const float* bp;
  const void* xb;
  void* z;
  float* cs_out;
  int64_t M;
  int32_t ldo, ldh, ldxb, ldz, C, inner;
  float eps;
} ls_ff_chain_desc;

int ls_ff_chain(const ls_ff_chain_desc* d, void* stream);

/*
 * The audio cross-attention branch of a BasicTransformerBlock, one launch (ABI 12;
 * attention.py:174-199 norm2 + attn2, Attention.forward :250-280 with the Whisper chunks
 * as encoder_hidden_states; replaces the LN-folded to_q GEMM + ls_attention + the
 * to_out GEMM with its residual):
 *   y = x + Wo softmax((Wq LN(x) + bq) K^T / sqrt(d)) V + bo
 * and stats_out = (mean, rstd) of the stored y rows (eps; norm3's LayerNorm fold).
 * x, y: bf16 rows [M][ldx] / [M][ldy], hw rows per image (a multiple of 128, M a multiple
 * of hw); ln_rowstats: (mean, rstd) of the x rows; kv: bf16 [M / hw * L][ldkv] rows of
 * to_k | to_v of the image's L audio tokens (L <= 64); wq / bq: packing.pack_xattn_q
 * (per head 48 rows with LayerNorm gamma / beta and log2(e) / sqrt(d) folded, k-images
 * swizzled); wo: packing.pack_xattn_wo (columns permuted to the kernel's k-slot order,
 * padding slots zero); bo: fp32 [C].  C = 320, 8 heads (the 32x32 level) only.
 */
typedef struct {
  const void* x;
  const float* ln_rowstats;
  const void* wq;
  const float* bq;
  const void* kv;
  const void* wo;
  const float* bo;
  void* y;
  float* stats_out;
  int64_t M;
  int32_t ldx, ldy, ldkv, C, heads, L, hw;
  float eps;
} ls_xattn_desc;

int ls_cross_attention_block(const ls_xattn_desc* d, void* stream);

/*
 * Small-M linear in fp32: y[m, n] = sum_k act(x[m, k]) * W[n, k] + bias[n]
 * (x fp32, W bf16 [N][K], 0 < M <= 1024, K <= 2048, K % 8 == 0); pre-activation SiLU optional.  TimestepEmbedding
 * (unet.py:382) and the batched time_emb_proj of every ResnetBlock3D
 * (resnet.py:190-194).
 */
int ls_small_linear(const float* x, int32_t M, int32_t K, const uint16_t* w, const float* bias, int32_t N,
                    int32_t silu_in, float* y, void* stream);

/* diffusers Timesteps(320, flip_sin_to_cos, shift) (unet.py:95,376): t read from
 * timesteps[*step] (device int32 array + device step index), out fp32 [B][dim]. */
int ls_timestep_embed(const int32_t* timesteps, const int32_t* step, int32_t B, int32_t dim, int32_t flip,
                      float shift, float* out, void* stream);

/* The same embedding for B fp32 timesteps, one per sample (ABI 13): the reference's
 * forward accepts a python float and a per-sample timestep vector, broadcasting it over
 * the batch (unet.py:361-376); ts device fp32 [B], out fp32 [B][dim]. */
int ls_timestep_embed_f32(const float* ts, int32_t B, int32_t dim, int32_t flip, float shift, float* out,
                          void* stream);

/*
 * CFG combine + DDIMScheduler.step (eta = 0) fused, then re-packs the next UNet
 * input (lipsync_pipeline.py:540-562).  eps: UNet output bf16 NHWC [Bu*P][ld_eps]
 * (4 used channels); lat fp32 [P][4] updated in place; coef fp32 table
 * [n_steps][4] = {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)} read at
 * *step; then *step += 1 (single thread).  When guidance > 1 the batch halves are
 * (uncond, audio).  unet_in (bf16 NHWC [Bu*P][ld_in]) receives the new latents in
 * channels 0..3 of every batch copy (8-byte stores: ld_in % 4 == 0, unet_in 8-B aligned;
 * channels 4.. of unet_in are left as they are).
 * LS_ERR_INVALID, nothing launched: null pointers, Bu other than 1 or 2, P < 1,
 * ld_eps < 4, ld_in < 4 or not a multiple of 4.
 */
int ls_ddim_cfg_step(const uint16_t* eps, int32_t ld_eps, int32_t Bu, int64_t P, float guidance, float* lat,
                     const float* coef, int32_t* step, uint16_t* unet_in, int32_t ld_in, void* stream);

/* Pixel prep (ImageProcessor.preprocess_fixed_mask_image image_processor.py:145-152):
 * faces uint8 NCHW [F][3][R][R]; mask fp32 [R][R] (1 = keep);
 * pix / masked bf16 NHWC [F][R][R][ld] (channels 3..ld-1 zeroed; ld 8 takes 16-byte
 * stores and needs 16-B aligned pix / masked).
 * LS_ERR_INVALID, nothing launched: null pointers, F < 1, R < 1, ld < 3. */
int ls_prep_pixels(const uint8_t* faces, int32_t F, int32_t R, const float* mask, uint16_t* pix, uint16_t* masked,
                   int32_t ld, void* stream);

/* DiagonalGaussianDistribution.sample + (z - shift) * scaling (lipsync_pipeline.py:296-297):
 * moments fp32 NHWC [P][ld_m] (mean = ch 0..3, logvar = ch 4..7), eps fp32 [P][4];
 * writes bf16 into dst[P][ld_dst] at channel offset c_off (channels c_off..c_off+3; the
 * others are left as they are).  logvar is clamped to [-30, 20] as the reference does.
 * LS_ERR_INVALID, nothing launched: null pointers, P < 1, ld_m < 8, c_off < 0 or
 * c_off + 4 > ld_dst. */
int ls_vae_sample(const float* moments, int32_t ld_m, const float* eps, int64_t P, float scaling, float shift,
                  uint16_t* dst, int32_t ld_dst, int32_t c_off, void* stream);

/* Builds the constant channels of the UNet input for a window
 * (lipsync_pipeline.py:517-549): ch 4 = nearest-resized keep-mask (prepare_mask_latents
 * :290), ch 5..8 masked-image latents, ch 9..12 reference latents (both already
 * written by ls_vae_sample into `cond` [P][16]); replicated into Bu copies of
 * unet_in [Bu][P][ld_in] together with the initial latents lat fp32 [P][4]; channels
 * 13..15 are zeroed, channels 16.. left as they are (P = F h h; two 16-byte stores per
 * pixel: unet_in 16-B aligned).
 * LS_ERR_INVALID, nothing launched: null pointers, F, R, h or Bu < 1, ld_in < 16 or not a
 * multiple of 8. */
int ls_pack_unet_input(const float* lat, const uint16_t* cond, const float* mask, int32_t F, int32_t R, int32_t h,
                       int32_t Bu, uint16_t* unet_in, int32_t ld_in, void* stream);

/* decode_latents prep (lipsync_pipeline.py:146-147): z = lat / scaling + shift,
 * lat fp32 [P][4] -> bf16 NHWC [P][ld] (channels 4..ld-1 zeroed; ld 8 takes 16-byte
 * stores and needs a 16-B aligned z).
 * LS_ERR_INVALID, nothing launched: null pointers, P < 1, ld < 4. */
int ls_scale_latents(const float* lat, int64_t P, float inv_scaling, float shift, uint16_t* z, int32_t ld,
                     void* stream);

/* paste_surrounding_pixels_back + pixel_values_to_images (lipsync_pipeline.py:327-341):
 * out = dec * (1 - keep) + pix * keep; dec / pix bf16 NHWC [F][R][R][ld*];
 * out_nchw fp32 [F][3][R][R] (may be NULL), out_u8 uint8 [F][R][R][3] (may be NULL):
 * out_u8 = trunc(clamp(out / 2 + 0.5, 0, 1) * 255).
 * LS_ERR_INVALID, nothing launched: null inputs, both outputs NULL, F < 1, R < 1, a pitch
 * below 3. */
int ls_paste_back(const uint16_t* dec, int32_t ld_dec, const uint16_t* pix, int32_t ld_pix, const float* mask,
                  int32_t F, int32_t R, float* out_nchw, uint8_t* out_u8, void* stream);

/* y[r, c] = x[r, c] + table[r % table_rows, c] (table fp32 [table_rows][C]): the
 * whisper positional-embedding add (whisper/model.py:155).  x / y rows are ldx / ldy elements
 * apart; columns C.. of y are left as they are.
 * LS_ERR_INVALID, nothing launched: null pointers, rows, C or table_rows < 1, ldx < C,
 * ldy < C. */
int ls_add_rows(const uint16_t* x, int64_t rows, int32_t C, int32_t ldx, const float* table, int32_t table_rows,
                uint16_t* y, int32_t ldy, void* stream);

/* Tuning / A-B switches for ls_conv2d (process-wide, host side only); any other key, or a value
 * a key does not take, is LS_ERR_INVALID:
 * key 1 = force the register-staged kernel (1) instead of the LDS-DMA one;
 * key 2 = force tile 0 auto, 1 128x128, 2 128x64, 3 64x64, 4 128x32, 5 256x256, 6 256x128,
 * 9 128x160; key 3 = split-K with key 2;
 * key 4 = ablation (1 skip MFMA, 2 skip operand DMA, 4 skip the output store, 8 the general epilogue
 * arithmetic; timing only);
 * key 6 = row-block GEMM on / off; key 7 = its K = 640 instances on / off; key 8 = halo-tile 3x3
 * conv on / off (ABI 12); key 9 = attention kernel variant: 0 only (the one there is);
 * key 12 = halo pieces over the read pixels only: 1 only; key 13 = 128-channel halo tiles where
 * 160 also divides N (measured slower; default off);
 * key 15 = K = 640 row-block GEMM with two 16-row fragments per wave (256-row blocks; default on);
 * key 16 = 128-column halo tiles on 16 x 8 patches, two blocks per CU, for Cin <= 256 (default on;
 * off: 16 x 16, one block per CU); key 17 = ls_ff_chain rows per wave: 1 (16 rows) only;
 * key 18 = nearest-x2 upsample convs on the halo-tile kernel (default on; off: the tiled gather);
 * key 19 = the narrow 16-column halo tile for 3x3 convs with N = 8 / 16 (the VAE's conv_out with
 * conv_norm_out + SiLU fused; default on; off: the tiled 128 x 32 GEMM); key 20 = the K = 640
 * residual linears on the row-block GEMM (default off: the tiled 128 x 160 kernel), always with
 * one fragment per wave (two with the residual tile do not fit the LDS);
 * (key 21 is not a key: it stays LS_ERR_INVALID;)
 * key 22 = the position-major form of the tiled 3x3 / stride 1 / pad 1 conv (ls_conv_plan_info.posmajor):
 * 0 never, 1 where its cost model prefers it to the standard raster (default), 2 wherever it is legal
 * (then also for calls that would run a 128-row tile; on 256 x 128 tiles for N < 256 or with key 2 = 6). */
int ls_set_tuning(int32_t key, int32_t value);

/* Diagnostics: workgroups per CU the runtime can co-schedule for a GEMM kernel
 * instance (hipOccupancyMaxActiveBlocksPerMultiprocessor with its dynamic LDS):
 * which 1 = 128x160 DMA tile, 2 = 256x256 8-wave tile, 3 = 128x128 DMA tile. */
int ls_gemm_occupancy(int32_t which);

/* Whisper log-mel spectrogram (whisper/audio.py:92-125: torch.stft n_fft 400, hop
 * 160, periodic Hann, centre/reflect padding, last frame dropped, |X|^2, mel
 * filterbank, log10 clamp 1e-10, clip-global max-8 floor, (x + 4) / 4).
 * audio fp32 [n_samples] (16 kHz mono), filters fp32 [n_mels][201];
 * out bf16 [t_pad][n_mels] frame-major, T = n_samples / 160 frames, zero for
 * T <= t < t_pad (the transcribe segment pad, whisper/audio.py pad_or_trim).
 * Workspace: ls_log_mel_workspace_bytes = 256 + T * n_mels * 4: the clip maximum (one
 * ordered uint32) at byte 0, the fp32 log10 mel rows [T][n_mels] before the floor at
 * byte offset 256; it is rewritten by every call and may hold anything before one. */
size_t ls_log_mel_workspace_bytes(int64_t n_samples, int32_t n_mels);
int ls_log_mel(const float* audio, int64_t n_samples, const float* filters, int32_t n_mels, int64_t t_pad,
               uint16_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* Sample-rate conversion by the rational factor L / M (sr_out / sr_in in lowest terms)
 * with a polyphase FIR: what ffmpeg does for the reference's read_audio (util.py:103-112)
 * and whisper's load_audio (whisper/audio.py:22-50).  x fp32 [n_in] mono; taps fp32
 * [L][2 * half + 1], row p = the filter of phase p (latentsync_amd.audio.resample_taps);
 * y fp32 [n_out], n_out = ceil(n_in * L / M).  Output n lies at input time n * M / L:
 *   base = (n * M) / L, p = (n * M) % L,
 *   y[n] = sum_{j = -half..half} taps[p][j + half] * x[base + j],  x = 0 outside [0, n_in)
 * (64-bit index arithmetic, zero padding by predicate, fp32 accumulation).  No
 * allocation, no synchronisation, capturable.  LS_ERR_INVALID, nothing launched: null
 * pointers, L, M, half or n_in < 1, n_out != ceil(n_in * L / M), L or M >= 2^22,
 * n_in > 2^40, or 255 * M / L + 2 * half + 2 > 16384 (the input window of one
 * 256-output block is staged in 64 KiB of LDS: M / L up to about 50). */
int ls_resample(const float* x, int64_t n_in, const float* taps, int32_t L, int32_t M, int32_t half, float* y,
                int64_t n_out, void* stream);

/* Audio2Feature.feature2chunks / get_sliced_feature (audio2feature.py:24-49, 85-100):
 * feat bf16 rows [T][layers][C] with row stride ld_row; chunk i, row j =
 * feat[clamp(int(i * 50 / fps) - 2 * left + j / layers, 0, T - 1)][j % layers];
 * out [n_chunks][(left + right + 1) * 2 * layers][C], bf16 or fp32 (out_f32). */
int ls_audio_chunks(const uint16_t* feat, int64_t ld_row, int32_t T, int32_t layers, int32_t C, int32_t n_chunks,
                    double fps, int32_t left, int32_t right, void* out, int32_t out_f32, void* stream);

/* ---- paste-back warp (restore_video), SURVEY.md §8(f) row 1 ---------------------- */

/* torchvision resize(face, (out_h, out_w), antialias=True) (aten _upsample_bilinear2d_aa)
 * followed by (x / 2 + 0.5).clamp(0, 1) * 255 -> uint8, as LipsyncPipeline.restore_video
 * does per face (lipsync_pipeline.py:348-354).  faces fp32 NCHW [N][3][in_h][in_w];
 * out uint8 HWC [N][out_h][out_w][3]. */
int ls_face_resize_u8(const float* faces, int32_t N, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                      uint8_t* out, void* stream);

/* ImageProcessor.resize on the ingest side (image_processor.py:42-44, 145-152; ABI 14):
 * torchvision's v1 transforms.Resize((out_h, out_w), BILINEAR, antialias=True) of a
 * uint8 face = cast to float, aten _upsample_bilinear2d_aa (width pass, then height
 * pass, float intermediate), torch.round (half to even), clamp to 0..255, uint8.
 * src uint8 NCHW [N][3][in_h][in_w] (data.pth "faces"); dst uint8 NCHW
 * [N][3][out_h][out_w].  A dimension that already matches is copied through.
 * LS_ERR_INVALID, nothing launched: null pointers, non-positive sizes, a downscale
 * factor above 7 in either dimension (the filter's taps are held in 16 registers). */
int ls_resize_faces_u8(const uint8_t* src, int32_t N, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                       uint8_t* dst, void* stream);

/* Constant tables of the warp (OpenCV initInterTab2D Lanczos4 fixed-point coefficients,
 * getGaussianKernel(2 w + 1, 0) for w = 0..w_edge_max), computed on the host and copied
 * into the caller's device buffer `tables` of ls_restore_tables_bytes(w_edge_max) bytes.
 * Synchronises `stream` (initialisation only; not capturable). */
size_t ls_restore_tables_bytes(int32_t w_edge_max);
int ls_restore_init_tables(void* tables, int32_t w_edge_max, void* stream);

/* AlignRestore.restore_img (affine_transform.py:85-115, upscale_factor 1) for N frames,
 * in place: frames uint8 [N][H][W][3]; faces uint8 [N][fh][fw][3] (the resized faces);
 * warp fp64 [N][6] = the frame->face matrix cv2.warpAffine iterates with (the inverse of
 * invertAffineTransform(affine_matrix), in warpAffine's own operation order);
 * roi int32 [N][4] (x0, y0, x1, y1), 16-byte aligned: the frame box outside which the
 * soft mask is 0 (width <= roi_w, height <= roi_h); w_edge_max bounds
 * int(sqrt(mask area)) // 20 and must not exceed the tables' bound.
 * Per pixel of the ROI: warpAffine(ones) bilinear -> 2x2 erode -> area (fp64) ->
 * (2 w_edge)^2 erode -> (2 w_edge + 1)^2 Gaussian (BORDER_REFLECT_101) -> soft;
 * frame = trunc(soft * mask_e * lanczos4(face) + (1 - soft) * frame).
 * Workspace: ls_restore_workspace_bytes(N, roi_h, roi_w). */
size_t ls_restore_workspace_bytes(int32_t N, int32_t roi_h, int32_t roi_w);
int ls_restore_frames(uint8_t* frames, int32_t N, int32_t H, int32_t W, const uint8_t* faces, int32_t fh, int32_t fw,
                      const double* warp, const int32_t* roi, int32_t roi_h, int32_t roi_w, int32_t w_edge_max,
                      const void* tables, void* workspace, size_t workspace_bytes, void* stream);

/* ---- face-alignment ingest + mask resize, SURVEY.md §8(f) row 2 / §8(a) a3 ----------- */

/* cv2.resize(img, (dst_w, dst_h), interpolation=INTER_LANCZOS4) for N uint8 HWC images
 * with C (1..4) interleaved channels: load_fixed_mask's mask.png resize
 * (image_processor.py:31-36) and the aligned face's resize to the resolution
 * (image_processor.py:141).  OpenCV's generic resize path (resize.cpp resizeGeneric_
 * with HResizeLanczos4 / VResizeLanczos4: int16 coefficients saturate_cast(c * 2048),
 * taps clamped to the image, (sum + 2^21) >> 22); dst_h == src_h and dst_w == src_w is
 * a copy, as in cv::resize.  The per-axis tables are built on the host and copied into
 * `workspace` (ls_resize_lanczos4_workspace_bytes): this call synchronises `stream`
 * (one-off preprocessing; not capturable). */
size_t ls_resize_lanczos4_workspace_bytes(int32_t dst_h, int32_t dst_w);
int ls_resize_lanczos4_u8(const uint8_t* src, int32_t N, int32_t src_h, int32_t src_w, int32_t C, uint8_t* dst,
                          int32_t dst_h, int32_t dst_w, void* workspace, size_t workspace_bytes, void* stream);

/* AlignRestore.align_warp_face (affine_transform.py:53-70): cv2.warpAffine(frame, M,
 * (out_w, out_h), INTER_LANCZOS4, BORDER_CONSTANT, border_value) for N uint8 RGB
 * frames [N][H][W][3] -> out [N][out_h][out_w][3].  warp fp64 [N][6] is the
 * dst->src matrix warpAffine iterates with (the inverse of M, in warpAffine's own
 * operation order); tables = the buffer of ls_restore_init_tables (its Lanczos-4
 * table). */
int ls_align_warp_u8(const uint8_t* frames, int32_t N, int32_t H, int32_t W, const double* warp, int32_t out_h,
                     int32_t out_w, int32_t border_value, const void* tables, uint8_t* out, void* stream);

/* ---- video writer, SURVEY.md §8(f) row 3 (additive, ABI stays 14) ------------------ */

/* Motion-JPEG encode of n RGB frames, uint8 [n][H][W][3] contiguous on the device (what
 * ffmpeg's encoder does for the reference's write_video, util.py:140-160).  Each frame
 * becomes the entropy-coded scan of one baseline JPEG: 8-bit, YCbCr 4:2:0 (MCU = Y0 Y1 Y2
 * Y3 Cb Cr), pixels past the right / bottom edge replicating the last column / row, the
 * Annex K quantisation tables scaled by the libjpeg quality rule (scale = 5000 / q below
 * 50, 200 - 2 q from 50; entry = clamp((base * scale + 50) / 100, 1, 255)), the Annex K
 * Huffman tables, a restart interval of ls_mjpeg_restart_interval() MCUs (DC predictors
 * reset, last byte padded with 1 bits, RSTm between intervals with m = interval index
 * mod 8, none after the last), 0x00 stuffed after every 0xFF.  Integer arithmetic
 * throughout (libjpeg's rgb_ycc_convert, h2v2_downsample, jpeg_fdct_islow and
 * quantiser), so the bytes are reproducible bit for bit.  The
 * caller adds the headers (SOI .. SOS) and EOI: latentsync_amd.video.jpeg_headers.
 *   out      uint8 [out_capacity]: the scans, frame after frame
 *   offsets  int64 [n + 1]: frame f occupies out[offsets[f] .. offsets[f + 1])
 * Bytes that would land at or past out_capacity are dropped while the offsets stay
 * exact, so offsets[n] > out_capacity tells the caller to retry with a larger buffer.
 * Frames are processed in batches of a fixed budget: the workspace
 * (ls_mjpeg_workspace_bytes) does not grow with n past one batch.  No allocation, no
 * synchronisation.  LS_ERR_INVALID, nothing launched: null pointers, quality outside
 * 1..100, n < 1, H or W outside 1..65535, more than 800000 MCUs per frame, negative
 * out_capacity (ls_mjpeg_workspace_bytes returns 0 for such sizes); LS_ERR_WORKSPACE:
 * workspace null or too small. */
int ls_mjpeg_restart_interval(void);
size_t ls_mjpeg_workspace_bytes(int32_t n, int32_t H, int32_t W);
int ls_mjpeg_encode(const uint8_t* frames, int32_t n, int32_t H, int32_t W, int32_t quality, uint8_t* out,
                    int64_t out_capacity, int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream);

/* ---- video reader, SURVEY.md §8(f) (additive, ABI stays 14) ------------------------- */

/* Motion-JPEG decode of n frames of one size into uint8 RGB [n][H][W][3] on the device:
 * the inverse of ls_mjpeg_encode for any 8-bit baseline JPEG with one interleaved scan
 * that is greyscale or YCbCr with chroma 1x1 and luma 1x1, 2x1 or 2x2.  The host parses
 * the segments in front of each scan (latentsync_amd.video.parse_jpeg); the device does
 * the rest, in libjpeg's integer arithmetic (jdhuff.c, jidctint.c jpeg_idct_islow with a
 * saturating range limit, jdsample.c fancy upsampling, jdcolor.c),
 * so the pixels equal libjpeg's bit for bit.
 *   data     uint8 [data_bytes]: the entropy-coded scans (anything may lie between them)
 *   frames   int64 [n][8] per frame: [0] first byte of its scan in data, [1] bytes from
 *            there to the end of its chunk (decoding stops after the last MCU, so an EOI or
 *            padding behind it is harmless), [2] restart interval in MCUs (0 = none),
 *            [3] sampling: 0 grey, 1 4:4:4, 2 4:2:2 (luma 2x1), 3 4:2:0 (luma 2x2),
 *            [4] quantiser index of component c in bits 16c..16c+15, [5] its DC and [6] its
 *            AC Huffman table index likewise, [7] 0
 *   quant    uint16 [n_quant][64]: quantiser steps in natural (row-major) order
 *   huff     int32 [n_huff][228]: per table, jdhuff.c's derived form -- uint16 [256]
 *            lookahead (length << 8 | symbol for every code of up to 8 bits, else 0),
 *            int32 [18] maxcode (by length; -1 = no code), int32 [18] valoffset, uint8 [256]
 *            huffval (video.huff_device_table builds it)
 *   max_segments  the largest number of restart segments of any frame (sizes the grid
 *            only: a smaller value is slower, never wrong)
 *   status   int32 [n]: 0, or why the frame could not be decoded -- 1 descriptor outside
 *            data, 2 RSTm markers missing, surplus or out of order, 3 a code longer than 16
 *            bits, 4 a coefficient index past 63, 5 a segment ran out before its MCUs.  The
 *            other frames of the call are unaffected; a refused frame's pixels are undefined.
 * No stream content makes the kernels read or write outside their buffers: every byte
 * index is checked against the segment's end and bytes past it are zero bits.  Frames are
 * processed in batches of a fixed budget: the workspace (ls_mjpeg_decode_workspace_bytes)
 * does not grow with n past one batch.  No allocation, no synchronisation.
 * LS_ERR_INVALID, nothing launched: null pointers, n < 1, H or W outside 3..65535,
 * negative data_bytes, table counts outside 1..65535 (ls_mjpeg_decode_workspace_bytes
 * returns 0 for such sizes); LS_ERR_WORKSPACE: workspace null or too small. */
size_t ls_mjpeg_decode_workspace_bytes(int32_t n, int32_t H, int32_t W);
int ls_mjpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* frames, int32_t n, int32_t H, int32_t W,
                    const uint16_t* quant, int32_t n_quant, const int32_t* huff, int32_t n_huff, int32_t max_segments,
                    uint8_t* out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- face brightness restore of use_darken requests (additive, ABI stays 14) --------- */

/* What the reference's write_video does to every output frame when `use_darken and
 * brightness_factor` (darken_restore.enhance_face_brightness, util.py:150-151), in place
 * on n RGB frames, uint8 [n][H][W][3] contiguous on the device.  DESIGN.md section 4.4 is
 * the definition: per detected frame a mask (two convex hulls filled, a dilate x dilate
 * box maximum with anchor dilate / 2, an n_taps Gaussian with BORDER_REFLECT_101, taps
 * added in index order with every product and sum rounded to float32), smoothed over
 * time (0.7 last + 0.3 mask; decaying by 0.8 over frames without a face), then every pixel
 * of a processed frame through OpenCV's 8-bit RGB -> HSV (hue range 180) -> RGB with
 * V' = clip(V (1 + g), 0, max_value) when `brighten`, else clip(V (1 - g), 0, 255), g = mask c.
 * The host half (latentsync_amd.darken) builds the tables:
 *   plan     int32 [n][4] on the device, per frame: [0] mode -- 0 leave the frame bit-identical,
 *            1 a detected frame with no mask before it, 2 a detected frame blended with the
 *            last mask, 3 no face: the last mask, which then decays, 4 no face and no mask yet:
 *            0.8 x the mask of frame `first_valid`; [1] its first vertex in verts, [2] the
 *            vertex count of hull A, [3] of hull B, which follows A (modes 1 and 2 only)
 *   verts    int32 [n_verts][2] on the device: hull vertices (x, y) in pixels, each hull
 *            strictly convex and ordered so that (b - a) x (p - a) >= 0 for consecutive
 *            vertices a, b and every inside point p; one or two vertices make a point or a
 *            segment.  A plan row that points outside verts gives an empty mask.
 *   first_valid  the frame (mode 1 or 2) whose mask serves mode 4, or -1
 *   roi_*    the region of interest: it holds every hull pixel inside the frame, grown by
 *            dilate + n_taps / 2; outside it the mask is exactly zero and is not computed
 *   taps     float [n_taps] on the device
 * Frames are processed in batches of frames_per_batch (0: a fixed budget); the workspace
 * (ls_face_brighten_workspace_bytes, 0 for sizes it refuses) holds the planes of one batch
 * plus the state carried across batches and does not grow with n.  No allocation, no
 * synchronisation.  LS_ERR_INVALID, nothing launched: null pointers, n < 1, H or W outside
 * 1..65535, n_taps even, below 1 or above 129, dilate < 1, max_value outside 0..255,
 * first_valid outside -1..n-1, a region of interest that is empty or not inside the frame;
 * LS_ERR_WORKSPACE: workspace null or too small. */
size_t ls_face_brighten_workspace_bytes(int32_t n, int32_t roi_h, int32_t roi_w, int32_t frames_per_batch);
int ls_face_brighten(uint8_t* frames, int32_t n, int32_t H, int32_t W, const int32_t* plan, const int32_t* verts,
                     int32_t n_verts, int32_t first_valid, int32_t roi_x, int32_t roi_y, int32_t roi_w, int32_t roi_h,
                     const float* taps, int32_t n_taps, int32_t dilate, float c, int32_t brighten, int32_t max_value,
                     int32_t frames_per_batch, void* workspace, size_t workspace_bytes, void* stream);

/* ---- StableSyncNet sync confidence (additive, ABI stays 14) --------------------------- */

/* The reference's SyncNet mel front end (latentsync/utils/audio.py:59-65 with
 * configs/audio.yaml), a different transform from ls_log_mel's Whisper one: audio fp32 mono
 * 16 kHz [n] -> out fp32 [T][80] frame-major, T = 1 + n / 200.  In this order:
 * pre-emphasis y[0] = x[0], y[i] = x[i] - 0.97 x[i-1]; STFT n_fft = win = 800, hop 200,
 * periodic Hann, centred with 400 ZEROS each side (librosa 0.10.1's default pad_mode);
 * magnitude; filters fp32 [80][401] (latentsync_amd.syncnet.mel_filters); S = 20 log10(max(
 * 1e-5, .)) - 20; clip(8 (S + 100) / 100 - 4, -4, 4).  fp32 throughout, a direct DFT
 * against a twiddle table.  One launch, no workspace.  LS_ERR_INVALID, nothing launched:
 * null pointers, n < 1 or above 2^38 (the frame count stays in int32). */
int ls_syncnet_mel(const float* audio, int64_t n, const float* filters, float* out, void* stream);

/* SyncNetDataset's visual input (syncnet_dataset.py, lower_half) from the pipeline's
 * aligned faces: faces uint8 [n][R][R][3] (run_windows' out_u8) -> out bf16
 * [B][R/2][R][3 F].  Window b holds frames starts[b] .. starts[b] + F - 1 (starts int32 [B]
 * on the device), rows R/2 .. R-1, channel 3 f + c ("b f c h w -> b (f c) h w"), value
 * (x / 255 - 0.5) / 0.5 in fp32 with an IEEE division, rounded to bf16.  The host checks
 * the starts; a window that leaves [0, n) is written as zeros and never read.
 * LS_ERR_INVALID: null pointers, n or B < 1, R odd, F < 1 or > n, 3 F % 8 != 0. */
int ls_syncnet_pack_frames(const uint8_t* faces, int32_t n, int32_t R, const int32_t* starts, int32_t B, int32_t F,
                           uint16_t* out, void* stream);

/* The audio encoder's input: mel fp32 [T][80] (ls_syncnet_mel) -> out bf16 [B][80][L][8],
 * channel 0 = mel[cols[b] + j][m] at pixel (m, j), channels 1..7 zero (the 1-channel conv_in
 * then runs on ls_conv2d with zero weight columns); cols int32 [B] on the device.  The host
 * checks cols[b] + L <= T; a column outside [0, T) is written as zero and never read.
 * LS_ERR_INVALID: null pointers, T, B or L < 1, L > T. */
int ls_syncnet_pack_mel(const float* mel, int32_t T, const int32_t* cols, int32_t B, int32_t L, uint16_t* out,
                        void* stream);

/* 3x3 convolution with one stride per axis and one-sided zero padding -- ResnetBlock2D's
 * anisotropic downsamplers (stable_syncnet.py:95-109, 129-131: F.pad then stride [1,2],
 * [2,1] or [2,3], padding 0) -- as an implicit GEMM on v_mfma_f32_16x16x32_bf16, fp32
 * accumulate: x bf16 NHWC [n_img][H][W] pitch ldx, y bf16 [n_img][Ho][Wo] pitch ldy,
 *   y[img, oy, ox, n] = bias[n] + sum_{ky, kx, ci} x[img, oy stride_h - pad_top + ky,
 *                                                   ox stride_w - pad_left + kx, ci] w[n, ky, kx, ci]
 * where a tap outside the image on ANY side reads zero (so Ho, Wo say how far the bottom /
 * right padding reaches).  w is ls_conv2d's packed 3x3 operand [N][K], K = 9 Cin rounded up
 * to 64, in the same two k orders (packing.pack_weight); bias fp32 [N] or NULL.  Any
 * M = n_img Ho Wo (also below 16) and any N.  A result does not depend on n_img: the kernel
 * form is chosen from K and N alone.  LS_ERR_INVALID, nothing launched: null x / w / y,
 * a stride outside 1..3, a pad outside 0..1, Cin % 8, ldx % 8, ldy % 8, ldx < Cin, ldy < N,
 * K not that of Cin, an output pixel whose first tap row or column is outside the image,
 * pointers not 16-byte aligned. */
int ls_conv3x3_strided(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t Cin,
                       const uint16_t* w, int32_t K, int32_t N, const float* bias, int32_t stride_h,
                       int32_t stride_w, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, uint16_t* y,
                       int32_t ldy, void* stream);

/* StableSyncNet.forward's tail and the score (stable_syncnet.py:55-60, 230-231): v_in, a_in
 * bf16 [B][D] (pitches ldv, lda): the encoders' norm_out outputs before the ReLU.  In fp32:
 * ReLU, x / max(|x|_2, 1e-12) (F.normalize) -> v, a fp32 [B][D] pitch ldo, and
 * score[b] = v . a / (max(|v|, 1e-8) max(|a|, 1e-8)) (F.cosine_similarity).  An all-negative
 * embedding gives a zero vector and score 0.  LS_ERR_INVALID: null pointers, B or D < 1,
 * a pitch below D. */
int ls_sync_score(const uint16_t* v_in, int32_t ldv, const uint16_t* a_in, int32_t lda, int32_t B, int32_t D,
                  float* v, float* a, int32_t ldo, float* score, void* stream);

/* ---- GIF thumbnail of a result, thumbnail.py of the reference (additive, ABI stays 14) -- */

/* cv2.resize(frame, (dw, dh), interpolation=INTER_AREA) for n uint8 RGB frames
 * [n][H][W][3] -> [n][dh][dw][3], downscale only (dh <= H, dw <= W).  As OpenCV defines it:
 * per axis scale = 1 / (dst / src) in fp64; destination index d covers the source cell
 * [d scale, (d + 1) scale) and takes the source samples it touches, a partial one weighted
 * by its covered fraction over the cell width (computeResizeAreaTab, weights cast to
 * fp32).  fp32 sums, the columns of one source row first (from 0), the rows second, one
 * rounding per multiply and per add, then saturate_cast<uchar> (round half to even).  When
 * both scales are integers: the integer sum of the cell times the fp32 1 / area, rounded
 * the same way ((sum + 2) >> 2 for 2 x 2).  One launch, no workspace, no synchronisation.
 * LS_ERR_INVALID, nothing launched: null pointers, n < 1, a size outside 1..65535, an
 * upscale on either axis. */
int ls_resize_area_u8(const uint8_t* src, int32_t n, int32_t H, int32_t W, uint8_t* dst, int32_t dh, int32_t dw,
                      void* stream);

/* Blends up to 16 layers into n uint8 RGB frames [n][H][W][3] in place, the same layers
 * into every frame.  `layers` is a HOST array int32 [n_layers][8] = {x0, y0, w, h, offset,
 * r, g, b} (it travels as a kernel argument): the layer covers the frame box [x0, x0 + w)
 * x [y0, y0 + h) (clipped to the frame; w or h 0: an empty layer) with the row-major uint8
 * alpha map alpha[offset .. offset + w h) on the device and the ink (r, g, b).  Every
 * pixel walks its layers in order with Pillow's blend, per channel
 *   t = ink a + dst (255 - a) + 128;  dst = ((t >> 8) + t) >> 8.
 * One launch (none when no layer has pixels).  LS_ERR_INVALID, nothing launched: null
 * frames, n, H or W < 1, n_layers outside 0..16, a negative w, h or offset, a map that
 * passes alpha_bytes, an ink outside 0..255, null layers / alpha where they are needed. */
int ls_overlay_blend_u8(uint8_t* frames, int32_t n, int32_t H, int32_t W, const int32_t* layers, int32_t n_layers,
                        const uint8_t* alpha, int64_t alpha_bytes, void* stream);

/* hist uint32 [32768]: the number of pixels of the n uint8 RGB frames [n][H][W][3] in each
 * 5-5-5 bin (r >> 3) << 10 | (g >> 3) << 5 | b >> 3.  The call zeroes hist first (a memset
 * on the stream); counts are exact.  LS_ERR_INVALID: null pointers, n, H or W < 1, more
 * than 2^32 - 1 pixels. */
int ls_rgb555_hist(const uint8_t* frames, int32_t n, int32_t H, int32_t W, uint32_t* hist, void* stream);

/* idx uint8 [n][H][W] = lut[5-5-5 bin of the pixel], lut uint8 [32768] on the device.
 * LS_ERR_INVALID: null pointers, n, H or W < 1. */
int ls_palette_map(const uint8_t* frames, int32_t n, int32_t H, int32_t W, const uint8_t* lut, uint8_t* idx,
                   void* stream);

/* GIF LZW (minimum code size 8: CLEAR 256, EOI 257, first code 258) of n index frames
 * uint8 [n][H][W]: the raw code bytes of every frame (before the split into 255-byte
 * sub-blocks, which the host does), LSB first, each frame padded to a whole byte.
 * A frame is cut into strips of ls_gif_strip_rows() rows (the last may be shorter), coded
 * independently and concatenated bit by bit into one ordinary stream: the first strip
 * starts with CLEAR; every strip starts from an empty dictionary at width 9; the width
 * grows when the decoder's next free code reaches 1 << width (no early change); once code
 * 4095 has been assigned the strip emits CLEAR (at width 12) and starts over; a strip ends
 * with its last code, then CLEAR -- EOI for the last strip of the frame -- at the width a
 * decoder has after that last code.
 *   out      uint8 [out_capacity]: frame after frame
 *   offsets  int64 [n + 1]: frame f occupies out[offsets[f] .. offsets[f + 1])
 * Bytes that would land at or past out_capacity are dropped while the offsets stay exact,
 * so offsets[n] > out_capacity tells the caller to retry with a larger buffer.  The
 * workspace (ls_gif_lzw_workspace_bytes; about 1.5 bytes per pixel) holds every strip's
 * worst case, (pixels + 2) codes of 12 bits, so no content can overflow it.  No
 * allocation, no synchronisation.  LS_ERR_INVALID, nothing launched: null pointers, n, H
 * or W outside 1..65535, negative out_capacity (ls_gif_lzw_workspace_bytes returns 0 for
 * such sizes); LS_ERR_WORKSPACE: workspace null or too small. */
int ls_gif_strip_rows(void);
size_t ls_gif_lzw_workspace_bytes(int32_t n, int32_t H, int32_t W);
int ls_gif_lzw(const uint8_t* idx, int32_t n, int32_t H, int32_t W, uint8_t* out, int64_t out_capacity,
               int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream);

/* ---- classic SyncNet evaluation (additive, ABI stays 14) ------------------------------ */

/* python_speech_features.mfcc(signal, 16000) with that library's defaults, from its
 * definition (the library is not a dependency; parity with it is unpinned): audio fp32 mono
 * 16 kHz [n] on the INT16 SCALE -> out fp32 [13][T] coefficient-major, T = 1 + ceil((n - 400)
 * / 160) for n > 400, else 1.  Pre-emphasis y[0] = x[0], y[i] = x[i] - 0.97 x[i-1]; frames of
 * 400 every 160, the tail zero-padded, rectangular window; |rfft(frame, 512)|^2 / 512; the
 * frame energy = its sum; filters fp32 [26][257] (latentsync_amd.synceval.mfcc_filters); a
 * zero energy becomes 2^-52; log; DCT-II ("ortho"), coefficients 0..12; lifter 1 + 11 sin(pi
 * k / 22); coefficient 0 = log(frame energy).  fp32 throughout, a direct DFT against a
 * twiddle table.  One launch, no workspace.  LS_ERR_INVALID, nothing launched: null
 * pointers, n < 1 or above 2^38. */
int ls_mfcc(const float* audio, int64_t n, const float* filters, float* out, void* stream);

/* Convolution over (time, y, x) as an implicit GEMM on v_mfma_f32_16x16x32_bf16, fp32
 * accumulate, for the windows ls_conv2d and ls_conv3x3_strided do not have: x bf16
 * [T][H][W][Cin] pitch ldx,
 *   y[t, oy, ox, n] = act(bias[n] + sum_{it, iy, ix, ci} x[t + it, oy stride_h - pad_h + iy,
 *                                                         ox stride_w - pad_w + ix, ci] w[n, it, iy, ix, ci])
 * for t < T - kt + 1, oy < Ho = (H + 2 pad_h - kh) / stride_h + 1, ox < Wo likewise; a tap in
 * the spatial padding reads zero; temporal stride 1, no temporal padding.  y is bf16
 * [T - kt + 1][Ho][Wo] pitch ldy, or fp32 with y_f32 = 1 (ldy in elements); act 0 none, 1
 * ReLU; bias fp32 [N] or NULL.  w is bf16 [N][K], k = ((it kh + iy) kw + ix) Cin + ci, K =
 * kt kh kw Cin rounded up to 64 with zero columns (packing.pack_weight_general).  With kt = 1
 * the T steps are independent images; a linear is kt = kh = kw = H = W = 1.  Any M (also
 * below 16) and any N.  The kernel form is chosen from K and N alone, so a result does not
 * depend on how many steps are computed together.  LS_ERR_INVALID, nothing launched: null
 * x / w / y, kt outside 1..5, kh or kw outside 1..7, a stride outside 1..2, a pad outside
 * 0..1, act or y_f32 outside 0..1, Cin % 8, ldx % 8, ldx < Cin, ldy < N, a bf16 ldy % 8, K
 * not that of the window, a window that does not fit (T < kt, H + 2 pad_h < kh, ...),
 * x / w / bf16 y not 16-byte aligned. */
int ls_conv_general(const uint16_t* x, int32_t ldx, int32_t T, int32_t H, int32_t W, int32_t Cin,
                    const uint16_t* w, int32_t K, int32_t N, const float* bias, int32_t kt, int32_t kh, int32_t kw,
                    int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w, int32_t act, void* y,
                    int32_t ldy, int32_t y_f32, void* stream);

/* Max-pool of bf16 NHWC [n_img][H][W][C] pitch ldx -> [n_img][Ho][Wo][C] pitch ldy, Ho =
 * (H + 2 pad_h - kh) / stride_h + 1: window 1..3, stride 1..2, pad 0..1 per axis (at most half
 * the window); the padding is -inf and never wins.  Exact.  LS_ERR_INVALID, nothing
 * launched: null pointers, a window / stride / pad outside those ranges, C % 8, a pitch % 8
 * or below C, a window that does not fit, pointers not 16-byte aligned. */
int ls_maxpool2d(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t kh,
                 int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w, uint16_t* y,
                 int32_t ldy, void* stream);

/* calc_pdist of syncnet_eval.py and its mean: im_feat, cc_feat fp32 [n][D] ->
 *   dists[i][j] = | im_feat[i] - ccp[i + j] + 1e-6 |_2   (F.pairwise_distance), fp32 [n][2 vshift + 1],
 * ccp = cc_feat with vshift rows of zeros at each end, and mean_dists[j] = mean_i dists[i][j],
 * fp32 [2 vshift + 1].  Every sum runs in a fixed order: the result is deterministic.  Two
 * launches.  LS_ERR_INVALID: null pointers, n outside 1..2^24, D < 1, vshift outside 0..15. */
int ls_sync_offset(const float* im_feat, const float* cc_feat, int32_t n, int32_t D, int32_t vshift, float* dists,
                   float* mean_dists, void* stream);

/* SyncNetDetector.crop_video's per-frame crop: frames uint8 RGB [n][H][W][3]; plan int32
 * [n][5] = (y0, y1, x0, x1, bsi) on the device.  Frame i is padded by bsi on every side with
 * the value 110, cropped to rows y0 .. y1 - 1 and columns x0 .. x1 - 1 of the padded frame and
 * resized to 224 x 224 as cv2.resize does by default for uint8 (INTER_LINEAR: 11-bit
 * fixed-point coefficients, two rounding passes; a 448 x 448 crop takes the 2 x 2 area mean)
 * -> out uint8 [n][224][224][3].  Written from OpenCV's definition; cv2 is not a dependency
 * and parity with it is unpinned.  A position outside the frame reads 110 wherever it lies;
 * an empty crop (the host refuses it) is written as zeros.  LS_ERR_INVALID: null pointers,
 * n < 1, a frame size outside 1..32768. */
int ls_crop_track(const uint8_t* frames, int32_t n, int32_t H, int32_t W, const int32_t* plan, uint8_t* out,
                  void* stream);

/* ---- S3FD face detector of the sync gate (additive, ABI stays 14) ---------------------- */

/* S3FD.detect_faces' input preparation: frames uint8 RGB [n][H][W][3] -> out bf16 [n][h][w][8],
 * h = round(H s), w = round(W s) (cvRound: half to even), resized as cv2.resize(image, (0, 0),
 * fx = s, fy = s, INTER_LINEAR) does for uint8 -- source step 1 / s on both axes, ls_crop_track's
 * 11-bit coefficients and two rounding passes; s = 1 copies -- minus the channel means: channel
 * 0 = R - 123, 1 = G - 117, 2 = B - 104 (the reference's two [2, 1, 0] swaps cancel), channels
 * 3..7 zero.  Integers below 256 in magnitude: exact in bf16.  Written from OpenCV's
 * definition; parity with cv2 itself is unpinned.  LS_ERR_INVALID, nothing launched: null
 * pointers, n < 1, a frame size outside 1..32768, s outside (0, 1], s = 0.5 (cv2 takes its
 * 2 x 2 area path there, which is not restated), an empty scaled frame, out not 16-byte
 * aligned. */
int ls_s3fd_prep(const uint8_t* frames, int32_t n, int32_t H, int32_t W, double s, uint16_t* out, void* stream);

/* The VGG trunk's convolution: 3 x 3, stride 1, padding = dilation (1 or 6), bias, ReLU, on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation; x bf16 [n_img][H][W][Cin] pitch ldx -> y bf16
 * [n_img][H][W][N] pitch ldy.  w is bf16 [N][9 Cin], k = (iy 3 + ix) Cin + ci
 * (packing.pack_weight_general of a 3 x 3 weight: ls_conv_general takes the same operand).  A
 * block owns 128 pixels x 64 channels and stages each (tap, 64-channel chunk) of w in LDS; a
 * tap in the padding is a zero operand and never a load, and a tap that is padding for a whole
 * block is skipped with its weights.  One kernel form for every shape, and a pixel's sum runs
 * in one fixed order: an image's result does not depend on n_img.  bias fp32 [N] or NULL.
 * LS_ERR_INVALID, nothing launched: null x / w / y, dilation not 1 or 6, Cin not a multiple of
 * 64 in 64..1024, N not a multiple of 64, a pitch % 8 or below its channel count, n_img / H / W
 * below 1, x / w / y not 16-byte aligned. */
int ls_conv3x3_relu(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t Cin,
                    const uint16_t* w, int32_t N, const float* bias, int32_t dilation, uint16_t* y, int32_t ldy,
                    void* stream);

/* MaxPool2d(2, 2, ceil_mode = True) of bf16 NHWC [n_img][H][W][C] pitch ldx -> [n_img][Ho][Wo][C]
 * pitch ldy, Ho = ceil(H / 2), Wo = ceil(W / 2); the last window of an odd axis is clipped to
 * the image.  Exact.  LS_ERR_INVALID, nothing launched: null pointers, C % 8, a pitch % 8 or
 * below C, n_img / H / W below 1, pointers not 16-byte aligned. */
int ls_maxpool2x2_ceil(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t C, uint16_t* y,
                       int32_t ldy, void* stream);

/* L2Norm.forward per pixel in fp32: y[p, c] = x[p, c] / (sqrt(sum_c x[p, c]^2) + 1e-10) weight[c];
 * x bf16 [M][C] pitch ldx -> y bf16 [M][C] pitch ldy, weight fp32 [C].  An all-zero row gives
 * zeros.  LS_ERR_INVALID, nothing launched: null pointers, C outside 8..8192 or % 8, a pitch %
 * 8 or below C, M < 1, pointers not 16-byte aligned. */
int ls_l2norm_scale(const uint16_t* x, int32_t ldx, int64_t M, int32_t C, const float* weight, uint16_t* y,
                    int32_t ldy, void* stream);

/* The tail of S3FDNet.forward and Detect.forward, one frame per block.  maps: a HOST array of
 * the six head maps on the device, fp32 NHWC [n][h_l][w_l][c_l] with loc and conf side by side:
 * c_0 = 4 + 4, c_l = 4 + 2 for l > 0; map_hw: a HOST array of the twelve sizes h_0, w_0, ...;
 * priors fp32 [P][4] on the device (cx, cy, w, h; PriorBox.forward computed in float64 on the
 * host), P = sum h_l w_l, level-major, row-major within a level.  Level 0's background logit is
 * the maximum of its conf channels 0..2; two-class softmax; decode() with variances (0.1, 0.2)
 * in the reference's operation order; the candidates are the scores > 0.05, of which exactly
 * the 5000 highest enter the greedy NMS (descending score, area (x2 - x1)(y2 - y1), a box stays
 * while IoU <= 0.3 with every kept one); out fp32 [n][750][5] = (score, x1, y1, x2, y2) in
 * normalised coordinates, the first 750 kept boxes, zero rows after counts[f] (int32 [n]):
 * the reference's output[:, 1].  keep_idx int32 [n][750] or NULL: the prior index of every kept
 * box, -1 after the count.  Equal scores order towards the lower prior index.  The workspace
 * (ls_s3fd_detect_workspace_bytes(n, P); 0 for sizes out of range) holds the sort keys and
 * decoded boxes.  No allocation, no synchronisation, one launch.  LS_ERR_INVALID, nothing
 * launched: null pointers, n outside 1..65535, P outside 1..65536 or not the maps' pixel
 * count, priors not 16-byte aligned; LS_ERR_WORKSPACE: workspace null, misaligned or too
 * small. */
size_t ls_s3fd_detect_workspace_bytes(int32_t n, int32_t P);
int ls_s3fd_detect(const float* const* maps, const int32_t* map_hw, int32_t n, const float* priors, int32_t P,
                   float* out, int32_t* counts, int32_t* keep_idx, void* workspace, size_t workspace_bytes,
                   void* stream);

/* The rest of S3FD.detect_faces: det fp32 [n][R][5] = (score, x1, y1, x2, y2) rows (ls_s3fd_detect's
 * out, or the per-scale lists of a frame one after the other).  Per frame the rows with score >
 * conf_th, in row order, times (frame_w, frame_h, frame_w, frame_h), then nms_ of box_utils.py:
 * descending score, areas (x2 - x1)(y2 - y1), a box stays while inter / (area_i + area_j - inter)
 * <= thresh against every kept one.  out fp32 [n][R][5] = (x1, y1, x2, y2, score) in nms_'s keep
 * order, zero rows after counts[f]; keep_idx int32 [n][R] or NULL: each kept box's index in
 * the frame's selected list, -1 after the count.  fp32 throughout (the reference runs nms_ in
 * float64 on the same fp32 values).  One launch.  LS_ERR_INVALID, nothing launched: null
 * pointers, n outside 1..65535, R outside 1..4096, a negative or NaN conf_th / thresh, a frame
 * size that is not positive. */
int ls_nms_boxes(const float* det, int32_t n, int32_t R, float conf_th, float frame_w, float frame_h, float thresh,
                 float* out, int32_t* counts, int32_t* keep_idx, void* stream);

int ls_abi_version(void);
const char* ls_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* LS_HIP_H */
