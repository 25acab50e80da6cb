/*
 * mi355audio.h -- C ABI of libmi355audio.so, the MI355X (gfx950 / CDNA4) kernel library
 * under the mlx-audio hot path (Kokoro-82M TTS: PL-BERT, bi-LSTM prosody predictor,
 * AdaIN / iSTFTNet vocoder; mlx_audio.dsp STFT / iSTFT / mel).
 *
 * The reference (Blaizzy/mlx-audio v0.5.0) has no FFI of its own: its operator boundary is the
 * Python `mlx.core` API.  Each entry point below therefore names the
 * `mlx.core` / `mlx.nn` call sites it replaces (file:line relative to the reference tree); the
 * Python layer `mlx_audio_amd` binds them with ctypes exactly as INTEGRATION.md shows.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the field name ends in `_host`;
 *   - activations are float32, channels-last: element (b, l, c) of a tensor lives at
 *     base + b*bstride + l*ld + c   (the NLC layout mx.conv1d uses), ld >= C;
 *   - `lens` (nullable) holds the valid row count of every batch item (ragged batches are padded
 *     to a common L; rows >= lens[b] read as zeros and are never written).  0 <= lens[b] <= L (T, Lin) is the
 *     caller's contract: the array lives on the device, so no entry point can check it without a
 *     synchronisation, and the kernels index rows, and LDS arrays sized by their documented maximum, by it;
 *   - weights are bfloat16 (or float16 for fp16 checkpoints), pre-packed by mi355_pack_* into MFMA fragment order;
 *   - `stream` is a hipStream_t passed as void*; all functions are asynchronous on it;
 *   - return value: 0 = ok, negative = error (text via mi355_last_error()); nothing is allocated,
 *     no global state is kept, distinct streams may be driven from distinct host threads.
 */
#ifndef MI355AUDIO_H
#define MI355AUDIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK 0
#define MI355_ERR_ARG (-1)
#define MI355_ERR_LAUNCH (-2)
#define MI355_ERR_UNSUPPORTED (-3)

const char* mi355_last_error(void);
/* ABI version of this header; bumped on any struct change. */
int mi355_abi_version(void);
/* Name/arch/CU count of device `dev` into caller buffers (used by bench.py). */
int mi355_device_info(int dev, char* name, int name_cap, int* cu_count, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * conv_gemm: conv1d / linear / polyphase conv_transpose1d as an implicit GEMM on MFMA
 * (v_mfma_f32_32x32x16_bf16; fp32 activations split on the fly into bf16 hi+lo so that the
 * result keeps ~16 mantissa bits, weights bf16; or v_mfma_f32_32x32x16_f16 on fp16-rounded activations).
 * Replaces: mx.conv1d / mx.conv_transpose1d in ConvWeighted (tts/models/kokoro/istftnet.py:
 * 128-170), nn.Conv1d (istftnet.py:771-786), nn.Linear (modules.py:15,60-90,477-600,
 * kokoro.py:84), the per-step x-projection mx.addmm of LSTM (modules.py:156-163), and the fused
 * neighbours the reference runs as separate MLX ops: AdaIN affine + Snake / LeakyReLU in front
 * (istftnet.py:337,379-380,907-908,818), bias / residual / scaling behind (istftnet.py:394,932,
 * 822,829).
 * ------------------------------------------------------------------------------------------ */
enum { MI355_ACT_NONE = 0, MI355_ACT_LEAKY = 1, MI355_ACT_SNAKE = 2, MI355_ACT_GELU = 3,
       MI355_ACT_ELU = 4,        /* prologue or epilogue: x > 0 ? x : expm1(x)  (Mimi SEANet, codec/models/mimi/modules/seanet.py) */
       MI355_ACT_SILU = 5,       /* epilogue */
       MI355_ACT_GELU_TANH = 6,  /* epilogue: nn.gelu_approx / GELU(tanh) */
       MI355_ACT_TANH = 7 };     /* epilogue */

typedef struct {
  /* input activation */
  const float* x;      /* [B, Lin, ldx] */
  int64_t x_bstride;   /* elements between batch items */
  int32_t ldx;         /* elements between rows (for the flattened strided conv: stride*Cin) */
  int32_t x_off;       /* element offset added to every row start (flattened conv: -pad*Cin) */
  int32_t Cin;         /* logical input channels per tap */
  int32_t Lin;         /* padded input rows */
  const int32_t* lens_in; /* [B] valid input rows, nullable => Lin */
  int32_t flat_valid;  /* 0: validity by row; >0: validity by flat element index in
                          [0, lens_in[b]*flat_valid)  (flat_valid = true channel count) */
  /* packed weights */
  const uint16_t* w;   /* from mi355_pack_conv_weight */
  int32_t Cout;        /* GEMM N (for conv_transpose: up_s * Cout_real) */
  int32_t K;           /* taps */
  int32_t dil;         /* dilation */
  int32_t pad;         /* left zero padding in rows */
  /* prologue: t = x*pre_scale[b,c] + pre_shift[b,c]; then activation */
  const float* pre_scale; /* [B, pre_ld] nullable */
  const float* pre_shift; /* [B, pre_ld] nullable (must be set iff pre_scale is) */
  int32_t pre_ld;
  int32_t pre_act;     /* MI355_ACT_NONE / LEAKY / SNAKE */
  float pre_slope;     /* leaky slope */
  const float* pre_alpha; /* [Cin padded to 32] snake alpha, nullable unless SNAKE */
  /* epilogue, in this order: v = act(acc + bias[n]) * colscale[n]; v += res; v += (accumulate ? old y : 0); y = v * out_scale
     (out_scale multiplies the accumulated value too: the BigVGAN / iSTFTNet stage mean sets out_scale = 1 / num_kernels on the LAST accumulating block only) */
  const float* bias;   /* [Cout] nullable */
  int32_t post_act;    /* MI355_ACT_NONE / LEAKY / GELU */
  float post_slope;
  const float* res;    /* residual [B, *, ldr], row = out_row >> res_shift; nullable */
  int64_t res_bstride;
  int32_t ldr;
  int32_t res_shift;
  float out_scale;     /* applied after the residual add */
  int32_t accumulate;  /* 1: y_new = y_old + value (resblock mean, istftnet.py:824-829) */
  float* y;            /* [B, Lout, ldy] */
  int64_t y_bstride;
  int32_t ldy;
  int32_t Lout;        /* GEMM rows per item (conv: output length; convT: Lin + K - 1) */
  const int32_t* lens_out; /* [B] valid GEMM rows, nullable => Lout */
  /* polyphase conv_transpose store: GEMM column n = r*up_cout + co is written to
     row u*up_s + r - up_p + up_row_off, column co, if 0 <= row < up_Lout (lens_up[b]) */
  int32_t up_s;        /* 0 = plain store */
  int32_t up_p;
  int32_t up_cout;
  int32_t up_row_off;
  int32_t up_Lout;
  const int32_t* lens_up; /* [B] nullable */
  int32_t B;
  int32_t precision;   /* 2 = bf16 hi+lo split (default; ~16 mantissa bits of the fp32 activation), 1 = single bf16 pass,
                          3 = single fp16 pass: activations rounded to fp16 (saturating), weights packed with MI355_W_F16,
                          4 = fp16 hi+lo split (~22 mantissa bits of the activation) on MI355_W_F16 weights: fp16 checkpoints
                              (Whisper) at fp32-activation accuracy,
                          5 = fp16 hi pass + block-scaled e4m3 lo pass on an MX image (mi355_pack_conv_weight_mx_host): the residual
                              t - fp16(t) (2^-11 of the value) and a second, e4m3 copy of the weights go through
                              v_mfma_scale_f32_32x32x64_f8f6f4 at twice the 16-bit rate, two taps per instruction, E8M0 scale per window
                              row and 32 channels / per output column: ~15 significant bits of the activation (conv sweep: <= 2e-5 of
                              the peak).  Launches the wave-specialised kernel does not take (few tiles, K % 4 != 3, thin outputs) run
                              the precision-4 arithmetic on the image's fp16 slices,
                          6 = fp16 hi pass + block-scaled FP4 (OCP e2m1) lo pass on an MX4 image (mi355_pack_conv_weight_mx4_host): as 5
                              with 4-bit elements on both sides of the lo product -- the matrix pipe runs them at 4x the 16-bit rate (the
                              lo pass costs ~0.27 of a 16-bit pass instead of ~0.55), the lo planes in LDS and the lo weight stream
                              halve; ~13 significant bits of the activation (waveform: ~4e-4 of the peak, 70 dB, against the 2e-3 /
                              50 dB bars: profiles/r6_split_format_study_fp6.txt).  Same eligibility and fallback as 5 */
  int32_t tile;        /* 0 = auto, else BM*1000+BN (128128, 64128, 64064), 6128128 / 6128064 (+ 10000000 * feature bits, + 100000000 *
                          ablation build) = the wave-specialised 8-wave kernel (ws4) on 128 x 128 / 128 x 64 tiles,
                          2064128 / 2064064 (+ 10000000 * groups) = split-K on 64-row tiles (needs split_ws) */
  /* optional instance-norm statistics of the STORED output, fused into the epilogue (plain stores only): per block of
     MI355_STATS_ROWS output rows and per channel the pair (sum, sum of squared deviations from the block mean), written
     (never accumulated) to stats_partial[b][row / MI355_STATS_ROWS][c][0..1]; consumed by mi355_adain_from_partials.
     Saves the separate read pass of InstanceNorm1d over the tensor this conv just produced (istftnet.py:173-338). */
  float* stats_partial;   /* nullable; [B, ceil(Lout / MI355_STATS_ROWS), Cout, 2] */
  int64_t stats_bstride;  /* elements between batch items */
  /* SnakeBeta prologue (Qwen3 codec decoder, speech_tokenizer.py SnakeBeta): with pre_act == MI355_ACT_SNAKE and
     pre_inv_beta set, t + pre_inv_beta[c] * sin^2(pre_alpha[c] * t)  (alpha = exp(log_alpha), inv_beta = 1/(exp(log_beta)+eps),
     evaluated once on the host); null = plain Snake with 1/alpha. */
  const float* pre_inv_beta; /* [Cin padded to 32] nullable */
  /* per-output-column scale applied after the epilogue activation and before the residual add (LayerScale:
     x + scale[c] * f(x), codec/models/mimi/modules/transformer.py LayerScale; ConvNeXt gamma). */
  const float* post_colscale; /* [Cout] nullable */
  /* optional workspace for launches of few output tiles (one utterance per call): with it the dispatcher may cut the input-channel range of a
     tile over several workgroups (fp32 partial tiles [B][groups][Lout][Cout] in the workspace) and apply the epilogue above in a second kernel
     that sums the groups in a fixed order.  NULL = never split.  The workspace is scratch of this call only (stream-ordered reuse is safe). */
  void* split_ws;
  int64_t split_ws_bytes;
  /* fake-quantised module input (KittenTTS activation_quant_modules, kitten_tts/quant.py:4-24): [B][2] = {-min, max} of the PROLOGUE'S OUTPUT over
     the utterance, both joined with 0, as mi355_fake_quant_extrema leaves them; the prologue then ends with the reference's dynamic uint8
     quantise / dequantise of every value (float32 op by op), so the quantised tensor is never materialised.  NULL = no quantisation. */
  const float* pre_fq;
  /* optional per-block extrema of the STORED output (round 5, ABI 33; KittenTTS): (min, max) per block of MI355_STATS_ROWS output rows and per channel,
     written (never accumulated) to ext_partial[b][row / MI355_STATS_ROWS][c][0..1], laid out like stats_partial.  The producer of a fake-quantised
     conv's input thereby hands over what that conv's extrema pass (mi355_fake_quant_extrema: one more read of the whole tensor) would compute: every
     quantised prologue in use is monotone per channel, so mi355_fake_quant_extrema_from_partials needs only these.  Produced by the quantising-prologue
     instantiations of the wave-specialised kernel (a fake-quantised model's convs feed fake-quantised convs): a launch with ext_partial set must
     satisfy mi355_conv_gemm_ext_supported and then always runs on that kernel. */
  float* ext_partial;     /* nullable; [B, ceil(Lout / MI355_STATS_ROWS), Cout, 2] */
  int64_t ext_bstride;    /* elements between batch items */
  /* pre-split activations (round 6, ABI 35): the wide linears of the transformer encoders (Whisper: 768 -> 768 / 2304 / 3072 at 96 000 rows) are bound
     by the producers' fp32 -> hi + lo conversion, which every one of the C_out / 128 column tiles of a row tile repeats
     (profiles/r6_conv_big_gemm_b64_call11.txt).  A SPLIT tensor has the layout of the fp32 tensor it replaces, each 32-bit word holding the 16-bit hi
     part of the value (bits 0-15) and the 16-bit lo residual (bits 16-31) in the type of the launch's precision (2: bfloat16, 4: IEEE half) -- exactly
     the two numbers the fp32 path's prologue would have produced, so both paths give the same bits.  x_split = 2 / 4: x holds split words (same
     strides; must equal `precision`; no prologue; wave-specialised kernel only: 16-byte aligned rows).  y_split = 2 / 4: the epilogue stores split
     words of its result instead of floats (for the launch that consumes y; res / accumulate / statistics still work on the float value).  Producers
     other than a conv epilogue: mi355_split16 (elementwise), mi355_layernorm (split field). */
  int32_t x_split;
  int32_t y_split;
} mi355_conv_gemm_args;
#define MI355_STATS_ROWS 64

int mi355_conv_gemm(const mi355_conv_gemm_args* a, void* stream);
/* What mi355_conv_gemm decides for a launch before it launches anything (an additive entry point: the ABI version stays).  Fields that do not apply to the family are 0. */
enum { MI355_ROUTE_4WAVE = 0, MI355_ROUTE_SPLITK = 1, MI355_ROUTE_WS4 = 2 };
typedef struct {
  int32_t family;        /* MI355_ROUTE_* */
  int32_t precision;     /* the arithmetic actually run (1 .. 6) */
  int32_t mx_fallback;   /* 1: an MX image (precision 5 / 6) on the precision-4 arithmetic of the 4-wave kernels */
  int32_t mx_lo_slices;  /* ... whose kernels skip this many e4m3 / FP4 tap-pair slices per chunk of the image */
  int32_t bm;
  int32_t bn;            /* tile rows and columns */
  int32_t vec;           /* 1: the 16-byte aligned input path */
  int32_t groups;        /* split-K: chunk groups */
  int32_t lean;          /* split-K: 1 = the lean finish kernel, 0 = the general one */
  int32_t gemm;          /* ws4: 1 = GEMM mode, 0 = conv mode */
  int32_t pre;           /* ws4: prologue kind (0 none, 1 LeakyReLU, 2 Snake, 3 SnakeBeta, 4 ELU) */
  int32_t epi;           /* ws4: epilogue family (0 none / LeakyReLU, 1 GELU, 2 SiLU, 3 GELU-tanh) */
  int32_t fq;            /* ws4: 1 = a quantising-prologue instantiation */
  int32_t two_by_two;    /* ws4: 1 = the precision-5 build with the 2 x 2 consumer layout */
  int32_t dbg;           /* ws4: 1 = the timeline-probe build */
  int32_t abl;           /* ws4: timing-ablation build (0 = none) */
  int32_t feat;          /* ws4: feature bits after the per-precision mask */
  /* ws4: the geometry that does not depend on the device (the grid is sized at launch time from the CU count and mi355_conv_ws4_resident) */
  int32_t tiles_per_item;
  int32_t P;
  int32_t NT;            /* row tiles per item, row tiles, column tiles */
  int32_t nch;
  int32_t keff;
  int32_t tap_rows;      /* chunks per tile, taps per chunk, LDS row shift per tap */
  int32_t R;             /* window rows */
  int32_t nslices;       /* weight slices of the packed image */
  int32_t fold;
  int32_t glog;
  int32_t total_ids;     /* residual folded into the accumulators, log2 of the XCD run length, virtual workgroup ids */
} mi355_conv_route;
/* Validates `a` and decides like mi355_conv_gemm, launches nothing and needs no device: *out = the route; a launch mi355_conv_gemm would refuse
 * returns that call's error code and mi355_last_error text and leaves *out alone.  No pointer of `a` is dereferenced. */
int mi355_conv_gemm_route(const mi355_conv_gemm_args* a, mi355_conv_route* out);
/* 1 = this launch can write ext_partial (pre_fq set, precision 2, plain store, a prologue / epilogue pair the wave-specialised kernel's quantising
 * instantiations carry, 16-byte aligned channels-last rows); 0 otherwise.  ext_partial itself need not be set in the probe. */
int mi355_conv_gemm_ext_supported(const mi355_conv_gemm_args* a);
/* Timeline probe of the wave-specialised kernel (tile code 46128128, tools/conv_timeline.py): device buffer of
 * [ceil(grid / 16)][8][4] uint64 s_memtime stamps (consumer wave 0 of every 16th workgroup, its first 8 tiles: tile start, first window
 * staged, main loop done, stores issued); NULL = off. */
int mi355_conv_ws4_debug_buffer(void* device_buffer);
/* Persistent workgroups the wave-specialised kernel's NEXT launches may take (process-wide, read on the host at launch time; 0 = default, two per
 * CU): lets independent convs of one stage run side by side on separate streams, each on a share of the CUs (the three resblocks of an MRF stage:
 * istftnet.py:797-835 loops over them one after the other). */
int mi355_conv_ws4_resident(int wgs);
/* Host-side packing (CPU, run once at load time).
 * w: float32 [Cout, K, Cin] in the MLX conv layout (values already weight-normed / bf16 rounded),
 * out: uint16 buffer of mi355_packed_conv_weight_elems(Cout, K, Cin) elements. */
int64_t mi355_packed_conv_weight_elems(int32_t Cout, int32_t K, int32_t Cin);
int mi355_pack_conv_weight_host(const float* w_host, int32_t Cout, int32_t K, int32_t Cin, uint16_t* out_host);
/* Same with an explicit element type: MI355_W_BF16 (precision 1 / 2) or MI355_W_F16 (precision 3; bf16-valued checkpoint
 * weights are exactly representable in fp16 down to 2^-17). */
enum { MI355_W_BF16 = 0, MI355_W_F16 = 1, MI355_W_FP8 = 2 };   /* MI355_W_FP8: row-major GEMV images only (mi355_pack_rowmajor_fp8_host) */
int mi355_pack_conv_weight_host_dt(const float* w_host, int32_t Cout, int32_t K, int32_t Cin, int32_t dtype, uint16_t* out_host);
/* The MX image of precision 5 (bf16-valued checkpoint weights are exact in its fp16 part): per 32-channel chunk K fp16 tap slices followed
 * by ceil(K / 2) e4m3 tap-pair slices, then one E8M0 scale byte per (padded) output column.  out_host: mi355_packed_conv_weight_mx_bytes bytes. */
int64_t mi355_packed_conv_weight_mx_bytes(int32_t Cout, int32_t K, int32_t Cin);
int mi355_pack_conv_weight_mx_host(const float* w_host, int32_t Cout, int32_t K, int32_t Cin, uint8_t* out_host);
/* The MX4 image of precision 6: the MX image's geometry and byte count (mi355_packed_conv_weight_mx_bytes), the tap-pair slots holding one kilobyte
 * of e2m1 codes per 32-column group (K block b of the matrix instruction = tap 2 p + b = lane half b) and the column scales of the 4-bit grid
 * (e[n] = floor(log2(max |w[n]|)) - 2). */
int mi355_pack_conv_weight_mx4_host(const float* w_host, int32_t Cout, int32_t K, int32_t Cin, uint8_t* out_host);

/* ------------------------------------------------------------------------------------------
 * Instance-norm statistics + AdaIN coefficients.
 * Replaces InstanceNorm1d / AdaIN1d (istftnet.py:173-338): per (b, c) mean / biased variance over
 * time, then scale = (1+gamma)*rsqrt(var+eps), shift = beta - mean*scale with
 * [gamma, beta] = fc(style) (computed by conv_gemm into `gb`).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t C; int32_t L; const int32_t* lens;
  int32_t B;
  double* sums;        /* workspace [B, C, 2], zeroed by the call */
  const float* gb;     /* [B, gb_ld]: gamma at [0,C), beta at [C,2C) */
  int32_t gb_ld;
  float eps;
  float* scale; float* shift; int32_t out_ld; /* [B, out_ld] */
  int32_t reuse_sums;  /* 1: `sums` already holds the statistics of this x (a previous call with the same x, lens): only the coefficients are
                          recomputed from another gb -- the three AdaINResBlock1 of a generator stage normalise the SAME input (istftnet.py:822-829) */
} mi355_adain_coef_args;
int mi355_adain_coef(const mi355_adain_coef_args* a, void* stream);

/* AdaIN coefficients from the per-block partial statistics a conv_gemm epilogue wrote (see stats_partial): merges the
 * blocks in float64 (Chan's parallel-variance formula; block row counts follow from lens / L), then the same
 * scale = (1+gamma)*rsqrt(var+eps), shift = beta - mean*scale as mi355_adain_coef. */
typedef struct {
  const float* partials; int64_t bstride;  /* [B, ceil(L / MI355_STATS_ROWS), C, 2] */
  int32_t C; int32_t L; const int32_t* lens; int32_t B;
  const float* gb; int32_t gb_ld; float eps;
  float* scale; float* shift; int32_t out_ld;
} mi355_adain_partials_args;
int mi355_adain_from_partials(const mi355_adain_partials_args* a, void* stream);

/* LayerNorm over the channel axis of rows, optionally fused with a residual add in front and
 * (1+gamma)*xhat+beta / weight*xhat+bias and LeakyReLU behind.
 * Replaces nn.LayerNorm (modules.py:35,445,481,523,537,551), AdaLayerNorm (modules.py:71-90). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;
  const float* res; int64_t res_bstride; int32_t ldr; /* nullable: normalise x + res */
  int32_t C; int32_t L; const int32_t* lens; int32_t B;
  const float* weight; const float* bias;   /* [C] nullable */
  const float* ada_gb; int32_t ada_ld;      /* [B, ada_ld]: gamma [0,C), beta [C,2C); nullable */
  float eps;
  int32_t post_act; float post_slope;
  float* y; int64_t y_bstride; int32_t ldy;
  int32_t y_split;   /* 0, or 2 / 4: y receives SPLIT words (mi355_conv_gemm_args.x_split of the linear that consumes it) instead of floats (ABI 35) */
} mi355_layernorm_args;
int mi355_layernorm(const mi355_layernorm_args* a, void* stream);
/* Elementwise fp32 -> SPLIT words (x_split of mi355_conv_gemm_args; fmt 2 = bfloat16 hi | lo << 16, 4 = IEEE half) over n contiguous values, n a
 * multiple of 4, both pointers 16-byte aligned; y may alias x.  For activations no conv epilogue / LayerNorm produces (attention outputs). */
int mi355_split16(const float* x, void* y, int64_t n, int32_t fmt, void* stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm with ONE group (ABI 37): per SAMPLE mean / biased variance over all (time x channel) elements, then a per-channel
 * weight and bias.  Replaces nn.GroupNorm(1, C, pytorch_compatible=True) behind every conv of the 48 kHz EnCodec
 * (codec/models/encodec/encodec.py:172-291, norm_type = "time_group_norm").  Three steps, so that the normalised tensor is
 * written only where something other than a conv prologue consumes it:
 *   statistics -> coefficients scale[b, c] = weight[c] * rstd[b], shift[b, c] = bias[c] - mean[b] * scale[b, c]
 *   (the shape of mi355_conv_gemm_args.pre_scale / pre_shift) -> apply.
 * ------------------------------------------------------------------------------------------ */
#define MI355_GN_PART_ELEMS 4096
/* Statistics pass: one read of x.  The valid elements of a sample (lens[b] rows of C channels) are cut into parts of
 * MI355_GN_PART_ELEMS consecutive elements, one workgroup each (a 1 s chunk of 48 000 x 32 floats is 375 workgroups); a part
 * leaves (sum, sum of squared deviations from the part's own mean) as two doubles.  Nothing is accumulated across workgroups:
 * mi355_group_norm_coef merges the parts in a fixed order. */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;   /* [B, L, ldx]; ldx == C reads 16 bytes per lane */
  int32_t C; int32_t L; const int32_t* lens; int32_t B;   /* lens [B] nullable => L */
  double* partials; int64_t partials_bstride;   /* [B, >= ceil(L * C / MI355_GN_PART_ELEMS), 2]; bstride in doubles */
} mi355_group_norm_stats_args;
int mi355_group_norm_stats(const mi355_group_norm_stats_args* a, void* stream);

/* Coefficients from partial statistics, merged in float64 with Chan's formula (first the total sum -> the mean, then
 * M2 = sum_e [M2_e + cnt_e (mean_e - mean)^2]).  conv_partials = 0: `partials` is what mi355_group_norm_stats wrote (doubles);
 * conv_partials = 1: `partials` is the stats_partial buffer of a mi355_conv_gemm epilogue, float [B, ceil(L / MI355_STATS_ROWS), C, 2],
 * merged over row blocks AND channels.  The coefficients are laid out `rep` times: scale[b, q * C + c] for q < rep (a strided conv
 * that reads regrouped rows [rows / rep, rep * C]); columns from rep * C to out_ld are zero. */
typedef struct {
  const void* partials; int64_t partials_bstride;   /* bstride in elements of the buffer's type */
  int32_t conv_partials;
  int32_t C; int32_t L; const int32_t* lens; int32_t B;
  const float* weight; const float* bias;   /* [C]; nullable => 1 / 0 */
  float eps;
  int32_t rep;         /* 0 => 1 */
  float* scale; float* shift; int32_t out_ld;   /* [B, out_ld], out_ld >= rep * C */
  float* mean_rstd;    /* nullable; [B, 2] */
} mi355_group_norm_coef_args;
int mi355_group_norm_coef(const mi355_group_norm_coef_args* a, void* stream);

/* y[b, l, c] = x0[b, l + row_off0, c] * scale0[b, c] + shift0[b, c]  (+ x1[b, l + row_off1, c] * scale1[b, c] + shift1[b, c]),
 * one pass, 16-byte accesses when C, the strides and the pointers allow.  scale1 == NULL with x1 set adds x1 as it is.
 * The two-operand form is the resnet block's shortcut_norm(...) + norm2(...); the row offset is the transposed conv's trim. */
typedef struct {
  const float* x0; int64_t x0_bstride; int32_t ldx0; int32_t row_off0;
  const float* scale0; const float* shift0;
  const float* x1; int64_t x1_bstride; int32_t ldx1; int32_t row_off1;   /* nullable */
  const float* scale1; const float* shift1;                              /* nullable (together) */
  int32_t coef_ld;     /* row stride of all coefficient arrays */
  int32_t C; int32_t L; int32_t B;   /* L = output rows */
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_group_norm_apply_args;
int mi355_group_norm_apply(const mi355_group_norm_apply_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * S3 speech tokenizer v2 (codec/models/s3/model_v2.py): the FSMN memory block and the FSQ head.  Two entry points added to
 * ABI 37 (new structs and functions only; no existing layout changed).  Plain float32, a fixed summation order that does not
 * depend on the launch geometry: two calls on the same bytes give the same bits.
 * ------------------------------------------------------------------------------------------ */
#define MI355_FSMN_MAX_TAPS 31
/* FSMNMultiHeadAttention.forward_fsmn (model_v2.py:152-172), channels-last.  For every b, t < L, c:
 *   y[b,t,c] = add[b,t,c] + m(b,t) * ( sum_{j<K} w[c,j] * m(b,t+j-left) * v[b,t+j-left,c] + v[b,t,c] ),
 * m(b,t) = (0 <= t < lens[b]), left = (K - 1) / 2, rows outside [0, L) read as zero.  v is usually the value third of a fused
 * q|k|v buffer (ldv = 3 C); add is the block's residual stream (NULL: the bare memory term).  K odd, <= MI355_FSMN_MAX_TAPS.
 * y must not alias v (y may be add). */
typedef struct {
  const float* v; int64_t v_bstride; int32_t ldv;       /* [B, L, ldv] */
  const float* add; int64_t add_bstride; int32_t add_ld; /* nullable; [B, L, add_ld] */
  const float* w;                                        /* [C, K] */
  int32_t K; int32_t C; int32_t L; const int32_t* lens; int32_t B;   /* lens [B] nullable => L */
  float* y; int64_t y_bstride; int32_t ldy;              /* [B, L, ldy] */
} mi355_fsmn_memory_args;
int mi355_fsmn_memory(const mi355_fsmn_memory_args* a, void* stream);

/* FSQCodebook.encode (model_v2.py:82-96): h = x w^T + b (8 outputs), codes[row] = sum_d (rint(tanhf(h_d) * 0.9990000128746033f) + 1) * 3^d
 * (round half to even, full-precision tanhf), one read of x.  With lens, rows = B * L and the rows at or beyond lens[b] give code 0
 * (and h = 0).  C a multiple of 4, <= 1280; x rows and w 16-byte aligned. */
typedef struct {
  const float* x; int32_t ldx; int64_t rows; int32_t C;  /* [rows, ldx] */
  const float* w; const float* b;                        /* [8, C]; [8] nullable => 0 */
  const int32_t* lens; int32_t L;                        /* nullable; lens [rows / L] */
  int32_t* codes;                                        /* [rows] */
  float* h;                                              /* nullable; [rows, 8] pre-activations */
} mi355_fsq_encode_args;
int mi355_fsq_encode(const mi355_fsq_encode_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * FastConformer encoder (stt/models/parakeet/attention.py, conformer.py): relative-position attention, the fused middle of the
 * convolution module and the 3 x 3 / stride 2 convs of the dw-striding subsampler.  Three entry points added to ABI 37 (new
 * structs and functions only; no existing layout changed).  Plain float32, a fixed summation order that does not depend on
 * the launch geometry: two calls on the same bytes give the same bits.
 * ------------------------------------------------------------------------------------------ */
/* RelPositionMultiHeadAttention (attention.py:93-137) behind the projections.  Head h sits at columns [h dh, (h + 1) dh) of
 * every row.  With n = lens[b] (NULL: T), for i, j < n:
 *   s_ij = scale * ( (q_i + u_h) . k_j + (q_i + v_h) . p[center - (i - j)] ),   out_i = sum_{j<n} softmax_j(s_i.) v_j;
 * output rows n <= i < T are written as zeros.  p is the PROJECTED position table [P, ldp], shared by the batch; row center is
 * distance 0 (rel_shift is out[i, j] = bd[i, T - 1 - i + j], so the row of a pair depends on i - j alone).  dh 64 or 128, T >= 1;
 * MI355_ERR_ARG without a launch unless 0 <= center - (T - 1) and center + T - 1 < P.  Rows 16-byte aligned (strides multiples of 4).
 * No [T, T] matrix is written to memory and there is no workspace. */
typedef struct {
  const float* q; int64_t q_bstride; int32_t ldq;        /* [B, T, ldq] */
  const float* k; int64_t k_bstride; int32_t ldk;
  const float* v; int64_t v_bstride; int32_t ldv;
  const float* p; int32_t ldp; int32_t P; int32_t center; /* [P, ldp] */
  const float* bias_u; const float* bias_v;              /* [heads * dh] */
  const int32_t* lens; int32_t B; int32_t T; int32_t heads; int32_t dh; float scale;
  float* out; int64_t out_bstride; int32_t ldo;          /* [B, T, ldo] */
} mi355_relpos_attention_args;
int mi355_relpos_attention(const mi355_relpos_attention_args* a, void* stream);

#define MI355_GLU_DWCONV_MAX_TAPS 31
/* Convolution.__call__ between its two pointwise convs (conformer.py:83-87), channels-last.  x [B, L, 2 C] is pointwise conv 1's
 * output; with g[t, c] = x[t, c] * sigmoid(x[t, C + c]) for 0 <= t < lens[b] and 0 elsewhere:
 *   z = b[c] + sum_{k<K} w[c, k] * g[t + k - (K - 1) / 2, c],   y[t, c] = z * sigmoid(z)   (full-precision expf),
 * rows lens[b] <= t < L are written as zeros.  w / b carry the depthwise bias and the BatchNorm running statistics, folded by the
 * caller.  K odd, <= MI355_GLU_DWCONV_MAX_TAPS; C a multiple of 4; y must not alias x. */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;        /* [B, L, ldx], ldx >= 2 C */
  const float* w; const float* b;                        /* [C, K]; [C] nullable => 0 */
  int32_t K; int32_t C; int32_t L; const int32_t* lens; int32_t B;   /* lens [B] nullable => L */
  float* y; int64_t y_bstride; int32_t ldy;              /* [B, L, ldy] */
} mi355_glu_dwconv_silu_args;
int mi355_glu_dwconv_silu(const mi355_glu_dwconv_silu_args* a, void* stream);

/* The 3 x 3 / stride 2 / pad 1 convs of DwStridingSubsampling (conformer.py:174-207), channels-last, To = (T - 1) / 2 + 1,
 * Fo = (F - 1) / 2 + 1:
 *   y[b, t, f, c] = act( bias[c] + sum_{kh,kw} w[c, kh, kw] * x[b, 2t + kh - 1, 2f + kw - 1, c * in_cstride] ),
 * in_cstride 0: x is [B, T, F] (the first conv's single input channel), 1: x is [B, T, F, C] (depthwise).  Input rows at or beyond
 * lens_in[b] and everything outside [0, T) x [0, F) read as zero; output rows at or beyond lens_out[b] are written as zeros. */
typedef struct {
  const float* x; int64_t x_bstride;                     /* [B, T, F (, C)] */
  const float* w; const float* bias;                     /* [C, 3, 3]; [C] nullable => 0 */
  int32_t B; int32_t T; int32_t F; int32_t C; int32_t in_cstride; int32_t relu;
  const int32_t* lens_in; const int32_t* lens_out;       /* [B] nullable => T / To */
  float* y; int64_t y_bstride;                           /* [B, To, Fo, C] */
} mi355_stencil2d_k3s2_args;
int mi355_stencil2d_k3s2(const mi355_stencil2d_k3s2_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sortformer (vad/models/sortformer/sortformer.py): attention of the BART-style Transformer encoder, 8 heads of 24.  One entry
 * point added to ABI 37 (new struct and function only; no existing layout changed).  Plain float32, a fixed summation order that
 * does not depend on the launch geometry: two calls on the same bytes give the same bits.
 * ------------------------------------------------------------------------------------------ */
/* TransformerAttention.__call__ (sortformer.py:532-564) behind the projections, under TransformerEncoder's key mask (621-631).
 * Head h sits at columns [h dh, (h + 1) dh) of every row.  With n = lens[b] (NULL: T), for i < n:
 *   out_i = sum_{j<n} softmax_j(scale * q_i . k_j) v_j;
 * output rows n <= i < T are written as zeros.  (The reference adds -1e4 to the scores of the keys j >= n; in float32 their
 * weights underflow to exactly 0 whenever a valid key exists, so hiding them is the same function.)  lens[b] >= 1 is the
 * caller's duty.  dh 8, 16, 24 or 32; any T >= 1; MI355_ERR_ARG without a launch for any other dh.  Rows 16-byte aligned (strides
 * multiples of 4).  No [T, T] matrix is written to memory and there is no workspace. */
typedef struct {
  const float* q; int64_t q_bstride; int32_t ldq;        /* [B, T, ldq] */
  const float* k; int64_t k_bstride; int32_t ldk;
  const float* v; int64_t v_bstride; int32_t ldv;
  const int32_t* lens; int32_t B; int32_t T; int32_t heads; int32_t dh; float scale;
  float* out; int64_t out_bstride; int32_t ldo;          /* [B, T, ldo] */
} mi355_narrow_attention_args;
int mi355_narrow_attention(const mi355_narrow_attention_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Moonshine (stt/models/moonshine/moonshine.py): attention for heads of 36 - 60 (tiny: 8 x 36, base: 8 x 52) and the partial
 * rotary embedding in front of it.  Two entry points added to ABI 37 (new structs and functions only; no existing layout
 * changed).  Plain float32, a fixed summation order: two calls on the same bytes give the same bits.
 * ------------------------------------------------------------------------------------------ */
/* MoonshineAttention.__call__ behind the projections: self, cross (Tq != Tk) and causal attention with grouped kv heads.
 * Head h sits at columns [h dh, (h + 1) dh) of the q / out rows and reads kv head h / (heads / kv_heads) of the k / v rows.
 * With nq = lens_q[b] (NULL: Tq) and nk = lens_k[b] (NULL: Tk), for i < nq:
 *   out_i = sum_j softmax_j(scale * q_i . k_j) v_j over the visible keys: j < nk, and under `causal` j <= i + (nk - nq)
 * (the queries are the last nq positions).  Invisible keys have probability exactly 0; a query with no visible key gives a zero
 * row; output rows nq <= i < Tq are written as zeros.  dh 36, 40, 44, 48, 52, 56 or 60; MI355_ERR_ARG without a launch for any
 * other dh, for Tq < 1 or Tk < 1, for heads % kv_heads != 0, for a row stride below heads * dh (kv_heads * dh for k / v) and for
 * rows that are not 16-byte aligned (strides multiples of 4).  Tq <= 4 runs one wavefront per (query, head, item) over any Tk
 * (the decode step); larger Tq runs 128-query tiles.  No [Tq, Tk] matrix is written to memory and there is no workspace. */
typedef struct {
  const float* q; int64_t q_bstride; int32_t ldq;        /* [B, Tq, ldq] */
  const float* k; int64_t k_bstride; int32_t ldk;        /* [B, Tk, ldk] */
  const float* v; int64_t v_bstride; int32_t ldv;
  const int32_t* lens_q; const int32_t* lens_k;          /* [B] nullable => Tq / Tk */
  int32_t B; int32_t Tq; int32_t Tk; int32_t heads; int32_t kv_heads; int32_t dh; int32_t causal; float scale;
  float* out; int64_t out_bstride; int32_t ldo;          /* [B, Tq, ldo] */
} mi355_mid_attention_args;
int mi355_mid_attention(const mi355_mid_attention_args* a, void* stream);

/* apply_rotary_pos_emb (moonshine.py:35-58): for every head of dh channels and every pair i < rot / 2
 *   (x[2i], x[2i+1]) -> (x[2i] c_i - x[2i+1] s_i, x[2i+1] c_i + x[2i] s_i),  c_i, s_i = cos / sin_table[(pos0 + l) * (rot / 2) + i],
 * each product rounded on its own; channels rot .. dh - 1 are copied.  x [B, L, ldx] holds `heads` heads from column 0; y may be x
 * (in place) or a cache slot.  The optional second operand (x2 -> y2, heads2 heads: the k heads into their cache row) is handled
 * by the same launch with the same positions.  Rows l >= lens[b] are left untouched.  rot even, 2 <= rot <= dh, dh % 4 == 0;
 * MI355_ERR_ARG without a launch when pos0 + L > rope_rows (positions past the tables). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t heads;
  float* y; int64_t y_bstride; int32_t ldy;
  const float* x2; int64_t x2_bstride; int32_t ldx2; int32_t heads2;   /* nullable */
  float* y2; int64_t y2_bstride; int32_t ldy2;
  int32_t dh; int32_t rot; int32_t B; int32_t L; int32_t pos0; int32_t rope_rows;
  const int32_t* lens;                                   /* [B] nullable => L */
  const float* cos_table; const float* sin_table;        /* [rope_rows, rot / 2] */
} mi355_partial_rope_args;
int mi355_partial_rope(const mi355_partial_rope_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bidirectional LSTM recurrence (the x-projection is a conv_gemm).
 * Replaces the per-time-step Python loops of LSTM._forward_direction/_backward_direction
 * (modules.py:150-240): gates i,f,g,o; c = f*c + i*g; h = o*tanh(c).
 * xp: [B, L, ldxp] gate pre-activations x@Wx^T + b_ih + b_hh, forward gates in columns [0,4H),
 * backward in [4H,8H).  wh: packed by mi355_pack_lstm_wh_host ([2][H/8][4H][8] bf16).
 * out: [B, L, ldo], forward h in columns [0,H), backward in [H,2H).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* xp; int64_t xp_bstride; int32_t ldxp;
  const uint16_t* wh; int32_t H;
  int32_t L; const int32_t* lens; int32_t B;
  float* out; int64_t out_bstride; int32_t ldo;
  int32_t quant_h;  /* 1: the recurrent product sees fake_quant_dynamic_u8(h) of each step's hidden vector; the emitted h is not quantised
                     * (KittenTTS LSTM with activation_quant, kitten_tts/modules.py:178,224) */
  int32_t wh_f16;   /* 1: wh holds IEEE half values (mi355_pack_lstm_wh16_host with f16 = 1: float32 checkpoints, 11 significant bits); 0: bf16 */
  float wh_scale;   /* with wh_f16: the packed values are W / wh_scale (wh_scale a power of two; 0 = 1): the recurrent sum is multiplied by it.  A bf16
                     * checkpoint scaled by 2^k into the normal range of IEEE half is held EXACTLY (8 significant bits), every fp32 product and sum is
                     * the unscaled one times 2^k, so the result is bit-identical to the bf16 image's -- at half the VALU work (v_fma_mix_f32 reads a
                     * half operand directly; a bf16 pair costs a shift / mask per weight on top of the FMA) */
} mi355_lstm_args;
int mi355_lstm_bidir(const mi355_lstm_args* a, void* stream);
int mi355_pack_lstm_wh_host(const float* wh_fwd_host, const float* wh_bwd_host, int32_t H, uint16_t* out_host);
/* same layout, element type chosen by f16 (0 = bf16 like mi355_pack_lstm_wh_host, 1 = IEEE half, round to nearest even) */
int mi355_pack_lstm_wh16_host(const float* wh_fwd_host, const float* wh_bwd_host, int32_t H, int32_t f16, uint16_t* out_host);

/* ------------------------------------------------------------------------------------------
 * Multi-head self-attention over short sequences (PL-BERT, T <= 512), fp32.
 * Replaces AlbertSelfAttention's QK^T / softmax / PV (modules.py:493-508).
 * qkv: [B, T, ld] with q at column 0, k at column D, v at 2D (D = heads*dh); keys >= lens[b]
 * get the reference's additive -10000 mask (weight exactly 0 in float32); query rows >= lens[b] of out are not written.
 * lens[b] <= T (<= 512) is the caller's contract (see Conventions): the probability row in LDS and the value rows are
 * indexed up to lens[b].
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* qkv; int64_t bstride; int32_t ld;
  int32_t heads; int32_t dh; int32_t T; const int32_t* lens; int32_t B;
  float* out; int64_t out_bstride; int32_t ldo;
} mi355_attention_args;
int mi355_attention(const mi355_attention_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small glue kernels of Kokoro's Model.__call__ (kokoro.py:111-177).
 * ------------------------------------------------------------------------------------------ */
/* y[b, l, 0:C] = table[idx[b, l], :] (+ table2[l, :] + row2[:]), rows >= lens[b] zeroed.
 * nn.Embedding (modules.py:24,429-431, 466-470) and the duration alignment gather that the
 * reference writes as a one-hot matmul (kokoro.py:161-169). */
typedef struct {
  const float* table; int32_t ld_table;          /* [rows, ld_table] or per-batch if table_bstride != 0 */
  int64_t table_bstride;
  const float* pos_table; int32_t ld_pos;        /* nullable: + pos_table[l, :] */
  const float* add_row;                          /* nullable: + add_row[:] */
  const int32_t* idx; int32_t idx_ld;            /* [B, idx_ld] */
  int32_t C; int32_t L; const int32_t* lens; int32_t B;
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_gather_rows_args;
int mi355_gather_rows(const mi355_gather_rows_args* a, void* stream);

/* k | v projection rows -> the 16-bit head-major blocks the decode-step attention streams (round 6, ABI 36; stt/models/whisper/whisper.py:360-365: the reference
 * computes k and v of the cross-attention once per window and caches them in the model's 16-bit dtype).  kv: float32 [B, T, ld] with G * H * dh value columns
 * (G groups -- k, v -- of H heads); out: [G, B, H, T, dh] of MI355_KV_BF16 / MI355_KV_F16, contiguous; round to nearest even.  One pass (read 4 bytes, write 2
 * per value) instead of a permute copy and a conversion copy per group.  dh a multiple of 8, ld a multiple of 4, 16-byte aligned pointers. */
int mi355_kv_head_major16(const float* kv, int64_t kv_bstride, int32_t ld, int32_t B, int32_t T, int32_t G, int32_t H, int32_t dh, void* out, int32_t out_dtype,
                          void* stream);

/* y[b, l, c] = v[b, c] for l < lens[b] (style broadcast, modules.py:393-395). */
int mi355_broadcast_rows(const float* v, int32_t ldv, int32_t C, float* y, int64_t y_bstride, int32_t ldy,
                         int32_t L, const int32_t* lens, int32_t B, void* stream);

/* duration head (kokoro.py:140-147): dur = clip(round(sum_j sigmoid(logits[b,t,j]) / speed), 1, 100),
 * then per item the exclusive scan and the frame->token index (kokoro.py:148-160).
 * frames[b] = sum of durations (the whole sum, also when it exceeds idx_ld); idx[b, f] = token of frame f (f < frames[b], up to idx_ld:
 * writes stop at the row end).  T <= 512 is checked; lens[b] <= T is the caller's contract (see Conventions): logits, dur and dur_raw rows
 * are indexed up to lens[b]. */
typedef struct {
  const float* logits; int64_t bstride; int32_t ld; int32_t bins;
  int32_t T; const int32_t* lens; int32_t B; float speed;
  const int32_t* forced_dur; /* nullable [B, T]: use these instead of the prediction */
  int32_t* dur;      /* [B, T] */
  float* dur_raw;    /* [B, T] nullable: pre-round value (tests check the rounding margin) */
  int32_t* frames;   /* [B] */
  int32_t* idx; int32_t idx_ld; /* [B, idx_ld], entries >= frames[b] untouched */
  int32_t max_frames; /* upper clip of one duration: 0 = 100 (Kokoro, kokoro.py:145-147); < 0 = none (KittenTTS, kitten_tts.py:398) */
} mi355_duration_args;
int mi355_duration_align(const mi355_duration_args* a, void* stream);

/* Dynamic per-tensor uint8 fake quantisation of one activation tensor per utterance (tts/models/kitten_tts/quant.py:4-24, the
 * ``maybe_fake_quant`` the KittenTTS modules apply to their inputs): y[b] = fq(act(scale[b,c] * x[b] + shift[b,c])) over the valid rows
 * of x [B, L, C] (rows >= lens[b] are neither read nor written).  The optional affine + activation prologue is what the consuming conv
 * would otherwise have fused (AdaIN + LeakyReLU / Snake): a quantised input has to exist in memory, because its extrema are needed first.
 * x == y is allowed.  ``minmax`` [B, 2] float32 is scratch (overwritten: {-min, max} per utterance). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t C; int32_t L; const int32_t* lens; int32_t B;
  const float* pre_scale; const float* pre_shift; int32_t pre_ld;   /* nullable pair [B, pre_ld] */
  int32_t pre_act; float pre_slope; const float* pre_alpha;          /* MI355_ACT_NONE / LEAKY / SNAKE (alpha [C]) */
  float* y; int64_t y_bstride; int32_t ldy;
  float* minmax;
} mi355_fake_quant_args;
/* {-min, max} per utterance of act(scale x + shift) from the per-block, per-channel extrema a producing conv left (mi355_conv_gemm_args.ext_partial):
 * here x = the partials [B, ceil(L / MI355_STATS_ROWS), C, 2], x_bstride = elements between items (ldx, y unused), everything else as in
 * mi355_fake_quant_extrema.  Per channel the prologue is evaluated at the channel's min and max (both ends: the affine slope may be negative) -- equal
 * to the sweep's result whenever the float32 evaluation of the prologue is monotone (always for the affine / LeakyReLU prologues; Snake's
 * x + sin^2(a x) / a has derivative 1 + sin(2 a x) >= 0 and can round non-monotonically by an ulp where that derivative vanishes, which moves the
 * quantiser's scale by <= 1e-7 relative). */
int mi355_fake_quant_extrema_from_partials(const mi355_fake_quant_args* a, void* stream);
int mi355_fake_quant_u8(const mi355_fake_quant_args* a, void* stream);
/* Extrema pass alone for a conv that quantises in its prologue (mi355_conv_gemm_args.pre_fq): minmax[b] = {-min, max} of act(scale x + shift)
 * over utterance b's valid rows, joined with 0; y is not touched (may be NULL).  The prologue value is evaluated exactly as the conv prologues
 * evaluate it (fmaf, v_sin, v_rcp + Newton), not with the libm calls of mi355_fake_quant_u8. */
int mi355_fake_quant_extrema(const mi355_fake_quant_args* a, void* stream);

/* Residual vector quantisation, encode side (codec/models/mimi/modules/quantization.py:37-45, 84-96: per layer argmin_b (|e_b|^2 / 2 - x . e_b),
 * first minimum, then x -= e_idx in float32): the quantiser of Mimi.encode (mimi.py:146-153; CSM audio context, sesame.py:527-559) and of the
 * Qwen3-TTS speech tokenizer's encoder (speech_tokenizer.py:1037-1058).  x is the PROJECTED input (after input_proj). */
typedef struct {
  const float* x; int64_t rows; int32_t ldx; int32_t D;      /* [rows, D] float32 */
  const float* tables;    /* [n_layers, bins, D]  embedding = embedding_sum / max(cluster_usage, 1e-5) */
  const float* tables_t;  /* [n_layers, D, bins]  the same values transposed (the search reads these) */
  const float* c2;        /* [n_layers, bins]     |e|^2 / 2 */
  int32_t bins; int32_t n_layers;
  int32_t* codes; int32_t ld_codes;   /* [rows, ld_codes >= n_layers] */
  float* margins;                     /* nullable, same layout as codes: second-best score - best score of every decision */
} mi355_rvq_encode_args;
int mi355_rvq_encode(const mi355_rvq_encode_args* a, void* stream);

/* ECAPA-TDNN speaker encoder of Qwen3-TTS (tts/models/qwen3_tts/speaker_encoder.py), the row-wise pieces between its convolutions (which are
 * mi355_conv_gemm launches).  mi355_ecapa_rows: y[b, r, c] = f(x[b, s, c]) * sigmoid(gate[b, c]) + res[b, s, c] with s = reflect(r - pad) for
 * r in [0, T + 2 pad): reflect_pad_1d (:11-26: mirror without repeating the edge row; needs pad < T), the Res2Net input "chunk + previous
 * output" (:98-101), the tanh in front of the attention conv (:213), SqueezeExcitationBlock's x * sigmoid(.) (:138-141) + the block residual (:180). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;        /* [B, T, C] float32, any row stride (a channel slice of a wider buffer) */
  const float* gate; int32_t gate_ld;                    /* nullable [B, C] LOGITS of the gate */
  const float* res; int64_t res_bstride; int32_t ldr;    /* nullable [B, T, C] */
  int32_t pre_tanh;                                      /* 1: f = tanh, 0: identity */
  float* y; int64_t y_bstride; int32_t ldy;              /* [B, T + 2 pad, C] */
  int32_t B; int32_t T; int32_t C; int32_t pad;
} mi355_ecapa_rows_args;
int mi355_ecapa_rows(const mi355_ecapa_rows_args* a, void* stream);
/* mean[b, c] = mean_t x[b, t, c];  std[b, c] (nullable) = sqrt(biased variance + eps)  (speaker_encoder.py:133, 201-202) */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;
  int32_t B; int32_t T; int32_t C;
  float eps;
  float* mean; float* std; int32_t out_ld;               /* [B, out_ld >= C] each */
} mi355_time_moments_args;
int mi355_time_moments(const mi355_time_moments_args* a, void* stream);
/* AttentiveStatisticsPooling's tail (speaker_encoder.py:219-228): w = softmax over TIME of logits[b, :, c];  out[b, c] = sum_t w x;
 * out[b, C + c] = sqrt(max(sum_t w (x - mean)^2, eps)). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;        /* [B, T, C] */
  const float* logits; int64_t l_bstride; int32_t ldl;   /* [B, T, C] */
  int32_t B; int32_t T; int32_t C;
  float eps;
  float* out; int32_t out_ld;                            /* [B, out_ld >= 2 C] */
} mi355_attentive_pool_args;
int mi355_attentive_pool(const mi355_attentive_pool_args* a, void* stream);

/* Anti-aliased activation of BigVGAN (codec/models/bigvgan/resample.py:157-177 ``Activation1d`` with SnakeBeta, activation.py:27-51):
 * x [B, L, C] channels-last -> y [B, L, C]:  2x up-sampling (edge pad 5, depthwise transposed conv with the 12-tap Kaiser-sinc filter, x 2, trimmed
 * to 2L: resample.py:101-136), a = u + inv_beta[c] * sin^2(alpha[c] * u), 2x down-sampling (edge pad 5 / 6, the 12-tap low-pass at stride 2:
 * resample.py:49-98, 139-154).  Ratio 2 and 12 taps only (the only configuration the reference builds).  up_filter / down_filter: 12 floats each on
 * the device (they are module buffers of the checkpoint); alpha, inv_beta: [C] (exp() of the log-scale parameters and 1 / (beta + 1e-9), applied at load). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t C; int32_t L; const int32_t* lens; int32_t B;
  const float* up_filter; const float* down_filter;
  const float* alpha; const float* inv_beta;
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_aa_act_args;
int mi355_aa_activation(const mi355_aa_act_args* a, void* stream);

/* Polyphase FIR sample-rate conversion (mlx_audio/resample.py:29-47 ``resample_audio_array`` = scipy.signal.resample_poly(x, up, down, window=taps,
 * padtype="edge") with the kaiser_best taps of resample.py:15-26; also utils.py:541-578 ``resample_audio``):  x [rows, n_in] -> y [rows, n_out],
 *   y[r][n] = sum_k table[k][p] * x[r][clamp(q - k, 0, n_in - 1)],   t = (n + first) * down,  p = t % up,  q = t / up.
 * table [K, up] float64 on the device (tap-major) = the taps x up, shifted right by (down - half % down) zeros (half = (len(taps) - 1) / 2; resample_poly
 * centres its output this way), split by phase: table[k][p] = padded[p + k * up], zero where that runs past the end; first = (half + shift) / down =
 * the outputs resample_poly drops at the front; n_out = ceil(n_in * up / down).  Sums are float64 like scipy's.  Two kernels: four same-phase outputs per
 * thread with a float32 input window in LDS when that window fits 64 KB (every pair of the usual rates), else one output per thread with a float64
 * window of (255 * down / up + K + 1) samples; a conversion that fits neither (384 kHz -> 8 kHz) is refused. */
typedef struct {
  const float* x; int64_t x_bstride; int32_t n_in; int32_t rows;
  const double* table; int32_t up; int32_t down; int32_t K; int32_t first;
  float* y; int64_t y_bstride; int32_t n_out;
} mi355_resample_args;
int mi355_resample_poly(const mi355_resample_args* a, void* stream);

/* AdaIN + LeakyReLU + depthwise ConvTranspose1d(k3, s2) with the first output dropped
 * (AdainResBlk1d pool, istftnet.py:879-881,907-915): x [B, L, C] -> y [B, 2L, C]. */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t C; int32_t L; const int32_t* lens; int32_t B;
  const float* scale; const float* shift; int32_t pre_ld; float slope;
  const float* w;    /* [C, 3] folded depthwise weight */
  const float* bias; /* [C] */
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_pool_up2_args;
int mi355_adain_pool_up2(const mi355_pool_up2_args* a, void* stream);

/* interpolate1d (tts/models/interpolate.py:61-132): x [rows, W] -> y [rows, size] (rows = N * C of the reference's [N, C, W]).
 * mode 0 = nearest: source index floor(i * scale) with scale = float32(W / size); mode 1 = linear with torch semantics: source coordinate
 * i * scale + half_scale - 0.5 clamped at 0 (scale = float32(W / size), half_scale = float32(0.5 * W / size)), or i * scale with
 * scale = float32((W - 1) / (size - 1)) when align_corners; every step rounded to float32 like the MLX op sequence. */
typedef struct {
  const float* x; int64_t x_rstride; int32_t W; int64_t rows;
  int32_t size; int32_t mode; int32_t align_corners; float scale; float half_scale;
  float* y; int64_t y_rstride;
} mi355_interp1d_args;
int mi355_interpolate1d(const mi355_interp1d_args* a, void* stream);

/* Scalar strided conv (1 -> 1 channel, k3, stride 2, pad 1) writing one column of a wider buffer:
 * Decoder.F0_conv / N_conv (istftnet.py:973-974,983-984).  x [B, Lin], y[b, l, col] for l < (lens_in[b] - 1) / 2 + 1; an item with
 * lens_in[b] = 0 has no output row (nothing is written for it). */
int mi355_conv1d_c1_k3s2(const float* x, int32_t ldx_b, int32_t Lin, const int32_t* lens_in,
                         float w0, float w1, float w2, float bias, float* y, int64_t y_bstride, int32_t ldy, int32_t col,
                         int32_t Lout, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------------
 * Harmonic source + STFT features + iSTFT head of the iSTFTNet Generator.
 * ------------------------------------------------------------------------------------------ */
/* SineGen + SourceModuleHnNSF (istftnet.py:548-709, 797-799): f0 [B, L2] at 2 values / frame ->
 * har_source [B, L2*up].  rand_ini [B, H] uniform, noise [B, L2*up, H] normal (explicit, so that
 * results are reproducible).  phase_ws: workspace [B, H, L2+1] floats. */
typedef struct {
  const float* f0; int32_t ld_f0; int32_t L2; const int32_t* lens2; int32_t B;
  int32_t up; int32_t H; float sr; float sine_amp; float noise_std; float voiced_thr;
  const float* rand_ini; const float* noise;
  const float* lin_w; float lin_b;  /* l_linear [H], bias */
  float* phase_ws;
  float* out; int32_t ld_out;
  float* quant_ws;  /* nullable [B, 2] scratch: when given, sine_wavs [L, H] goes through fake_quant_dynamic_u8 (per utterance) before l_linear
                     * (KittenTTS with activation_quant on m_source.l_linear, kitten_tts/istftnet.py:711-713) */
  int32_t coarse_f32; /* 1: coarse-grid length = ceil(L * float32(1 / up)) = L2 + 1 (KittenTTS hands interpolate() a float32 scale factor,
                       * kitten_tts/istftnet.py:572,595-599); 0: ceil(L * (1.0 / up)) in doubles (Kokoro, istftnet.py:567,590-594) */
} mi355_sine_source_args;
int mi355_sine_source(const mi355_sine_source_args* a, void* stream);

/* MLXSTFT.transform (istftnet.py:473-506) for small n_fft (<= 64): reflect-centred STFT with a
 * caller-supplied window, magnitude and atan2 phase, written channels-last:
 * x [B, L] -> y[b, f, 0:nb] = |X|, y[b, f, nb:2nb] = angle(X), f in [0, L/hop], nb = n_fft/2+1.
 * Precondition: L > n_fft/2 (checked) and, with lens, lens[b] > n_fft/2 for every item (NOT checked: lens lives on the device) -- the
 * reflect padding is one reflection; below that the kernels clamp the index into the item and the values are not the reference's.
 * Item b gets rows f in [0, lens[b]/hop]; rows past that are left untouched. */
typedef struct {
  const float* x; int32_t ldx; int32_t L; const int32_t* lens; int32_t B;
  int32_t n_fft; int32_t hop; const float* window;
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_stft_magphase_args;
int mi355_stft_magphase(const mi355_stft_magphase_args* a, void* stream);

/* Generator tail (istftnet.py:830-835 + MLXSTFT.inverse :508-541 + dsp.istft :436-513 with
 * normalized=True, center=True): x [B, Fr, 2nb] (conv_post output) -> spec = exp(x[..., :nb]),
 * phase = sin(x[..., nb:]), irfft, synthesis window, w^2 overlap-add as a gather,
 * trim n_fft/2 each side -> audio [B, (Fr-1)*hop]. */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t Fr; const int32_t* lens; int32_t B;
  int32_t n_fft; int32_t hop; const float* window;
  float* audio; int32_t ld_audio;
} mi355_istft_head_args;
int mi355_istft_head(const mi355_istft_head_args* a, void* stream);

/* The whole generator tail in ONE launch (new struct and function only; ABI stays 37): conv_post behind its LeakyReLU
 * (istftnet.py:830-831, `x = leaky_relu(x); x = conv_post(x)`) plus the exp / sin / MLXSTFT.inverse of the generator's forward
 * (istftnet.py:832-835, :508-541; dsp.istft dsp.py:436-513) -- i.e. mi355_conv_gemm(pre_act = LEAKY, K = 7, pad = 3, precision 2) followed by
 * mi355_istft_head, without the [B, Fr, 2 nb] tensor between them.  x [B, L, Cin] float32 (rows 16-byte aligned), w / bias: the conv's
 * packed bf16 image (mi355_pack_conv_weight_host; n-tile 0 is read, columns >= Cout are zero in it) and fp32 bias (nullable),
 * audio [B, (L - 1) * hop].  Item b uses rows [0, lens[b]) (rows outside read as zero AFTER the LeakyReLU, as the conv's padding) and
 * gets samples [0, (lens[b] - 1) * hop); samples beyond are left untouched.  The arithmetic per output value is that of the two launches
 * (bf16 hi + lo passes, chunk -> tap order, bias, then the head's own steps); the path does not depend on B or on the number of blocks.
 * Supported: Cin % 32 == 0, K == 7, dil == 1, pad == 3, n_fft == 20, hop == 5, Cout == 2 * (n_fft / 2 + 1) <= 32, pre_act == MI355_ACT_LEAKY,
 * precision == 2; anything else returns MI355_ERR_UNSUPPORTED without a launch (the caller keeps the two launches). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t Cin; int32_t L; const int32_t* lens; int32_t B;
  const uint16_t* w; const float* bias; int32_t Cout; int32_t K; int32_t dil; int32_t pad;
  int32_t pre_act; float pre_slope; int32_t precision;
  int32_t n_fft; int32_t hop; const float* window;
  float* audio; int32_t ld_audio;
} mi355_conv_post_istft_args;
int mi355_conv_post_istft(const mi355_conv_post_istft_args* a, void* stream);

/* One up-sampler of the generator in ONE dedicated launch (new struct and function only; ABI stays 37): `x = leaky_relu(x, 0.1); x = ups[i](x);
 * x = x + x_source` (istftnet.py:161-166, :811-826) -- i.e. the polyphase mi355_conv_gemm call (pre_act = LEAKY, K / u = 2 taps, pad = 1,
 * res = x_source, up_s = u, up_p = p, up_cout = Cout, up_row_off = row_off, precision 2) on a kernel whose workgroups own a block of input rows
 * and ALL u * Cout columns of it, so the activation window is loaded, activated and split once.  x [B, L, Cin] float32 (rows 16-byte aligned),
 * w / bias: the polyphase bf16 image of mi355_pack_conv_weight_host ([u * Cout, 2, Cin], ops.pack_conv_transpose) and the fp32 bias [Cout]
 * (nullable); res, y [B, L * u + row_off, Cout].
 *   y[b, row_off + u m + phase - p, :] = sum over taps leaky(x[b, m - 1 + tap, :]) W[phase, tap] + bias + res[b, same row, :]
 * for the output rows [row_off, row_off + lens[b] * u); input rows >= lens[b] read as zero AFTER the LeakyReLU, output rows beyond are left
 * untouched.  row_off = 1 (the last stage, whose output carries one zero left-pad row): y[b, 0, :] = res[b, 0, :] as well.  Per output value the
 * arithmetic and its order are those of mi355_conv_gemm's wave-specialised kernel (bf16 hi + lo passes, chunk -> tap order, bias, residual):
 * bit-equal results; the path does not depend on B or L.
 * Supported: (Cin, Cout, u) = (512, 256, 10) or (256, 128, 6), K == 2 u, p == (K - u) / 2, row_off 0 / 1, precision == 2; anything else returns
 * MI355_ERR_UNSUPPORTED without a launch (the caller keeps mi355_conv_gemm). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t Cin; int32_t L; const int32_t* lens; int32_t B;
  const uint16_t* w; const float* bias; int32_t Cout; int32_t K; int32_t u; int32_t p; int32_t row_off;
  float slope; int32_t precision;
  const float* res; int64_t res_bstride; int32_t ldr;
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_upsample_polyphase_args;
int mi355_upsample_polyphase(const mi355_upsample_polyphase_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * mlx_audio.dsp (dsp.py): batched STFT / iSTFT for arbitrary n_fft (mixed-radix 2/3/4/5 +
 * generic-prime Stockham FFT staged in LDS) and the fused |X|^2 -> mel -> log front ends.
 * ------------------------------------------------------------------------------------------ */
/* dsp.stft (dsp.py:385-433): x [B, L] (already centre-padded by the caller or pad_mode applied
 * here: 0 none, 1 reflect, 2 constant) -> out complex64 [B, n_frames, n_fft/2+1] interleaved. */
typedef struct {
  const float* x; int32_t ldx; int32_t L; int32_t B;
  int32_t n_fft; int32_t hop; const float* window; /* [n_fft] already zero-padded */
  int32_t pad_mode; int32_t n_frames;
  float* out;  /* [B, n_frames, n_fft/2+1, 2] */
} mi355_stft_args;
int mi355_stft(const mi355_stft_args* a, void* stream);

/* Fused STFT -> power/magnitude -> mel -> log (whisper/audio.py:41-82; qwen3_tts.py:64-120).
 * mode 0 (whisper): p = |X|^2, y = log10(max(mel, 1e-10)) (global max clamp + (y+4)/4 by
 *   mi355_logmel_finish); mode 1 (qwen3): p = sqrt(|X|^2 + 1e-9), y = log(max(mel, 1e-5)); mode 2 (kaldi fbank): p = |X|^2,
 *   y = log(max(mel, 1e-8)); mode 3 (vocos, codec/models/vocos/mel.py:9-33): p = |X|, y = log(max(mel, 1e-5));
 *   mode 4 (NeMo FilterbankFeatures: stt/models/parakeet/audio.py:71-79, vad/models/sortformer/sortformer.py:95-97): p = |X|^2,
 *   y = log(mel + log_guard).
 * fb: [n_mels, n_fft/2+1] float32.  out [B, n_frames, n_mels]. */
typedef struct {
  const float* x; int32_t ldx; int32_t L; int32_t B;
  int32_t n_fft; int32_t hop; const float* window; int32_t pad_mode; int32_t n_frames;
  const float* fb; int32_t n_mels; int32_t mode;
  float* out;
  float* gmax;  /* [B] running max for mode 0 (must be -inf initialised by the call), nullable */
  float log_guard;  /* mode 4: the additive guard inside the log (NeMo's log_zero_guard_value, 2^-24) */
} mi355_logmel_args;
int mi355_logmel(const mi355_logmel_args* a, void* stream);
int mi355_logmel_finish(float* y, int64_t n_per_item, const float* gmax, int32_t B, void* stream);

/* Kaldi framing for dsp.compute_fbank_kaldi (dsp.py:821-975): frame f covers x[f*shift - pad, +win) with Kaldi's edge reflection
 * (snip_edges=True: pad = 0), + dither * noise (nullable), - frame mean, pre-emphasis inside the frame, * window, zero-padded to n_fft.
 * frames [n_frames, n_fft] then goes through mi355_logmel with mode 2 (|X|^2 -> mel -> log(max(., 1e-8))), hop = n_fft, window = ones. */
typedef struct {
  const float* x; int32_t L;
  int32_t win; int32_t shift; int32_t pad; int32_t n_fft; int32_t n_frames;
  const float* window;   /* [win] */
  const float* noise;    /* [n_frames, win] standard normal, nullable */
  float dither; float preemph;
  float* frames;         /* [n_frames, n_fft] */
} mi355_kaldi_frames_args;
int mi355_kaldi_frames(const mi355_kaldi_frames_args* a, void* stream);
/* Vocos ISTFTHead, first half (codec/models/vocos/vocos.py:126-134: mag, p = split(out(x)); mag = clip(exp(mag), max 1e2);
 * S = mag * (cos p + 1j sin p)): x [B, Fr, 2 nb] float32 (row pitch ldx) -> spec [B, Fr, nb] complex64 (interleaved re, im), which
 * mi355_istft then inverts (dsp.istft, plain-window overlap-add normalisation). */
int mi355_polar_spec(const float* x, int64_t x_bstride, int32_t ldx, int32_t Fr, int32_t nb, int32_t B, float clip, float* spec, void* stream);


/* dsp.istft / ISTFTCache.istft (dsp.py:436-513, 663-738): spec [B, n_frames, nb, 2] ->
 * frames irfft(n_fft) * window, overlap-add (gather form), / norm[t] (precomputed window
 * envelope), out[b, t - trim] for t in [trim, trim+out_len).  clamp: constrain_value_range. */
typedef struct {
  const float* spec; int32_t n_frames; int32_t B;
  int32_t n_fft; int32_t hop; const float* window; const float* norm; /* [ola_len] */
  int32_t norm_mode;  /* 0: out/norm always (ISTFTCache); 1: divide only where norm > 1e-10 (dsp.istft) */
  int32_t clamp; int32_t trim; int32_t out_len;
  float* frames_ws;   /* workspace [B, n_frames rounded up to even, n_fft] floats */
  float* out; int32_t ld_out;
} mi355_istft_args;
int mi355_istft(const mi355_istft_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scaled-dot-product attention with GQA, causal / sliding-window masks and ragged lengths, exact f32
 * (v_mfma_f32_32x32x2_f32 flash kernel for Tq > 8, a KV-cache streaming kernel for decode steps).
 * Replaces Whisper MultiHeadAttention.qkv_attention (stt/models/whisper/whisper.py:371-385: q@k, + mask,
 * softmax(precise=True), w@v) and mx.fast.scaled_dot_product_attention under the Qwen3-TTS talker / code predictor /
 * codec transformer (tts/models/qwen3_tts/talker.py:307, speech_tokenizer.py:150-186), the Mimi transformer
 * (codec/models/mimi/modules/transformer.py:96-113) and the CSM Llama blocks (tts/models/sesame/attention.py:150-175).
 * q [B, Tq, ldq] with head h at columns [h*dh, (h+1)*dh); k, v [B, Tk, ldk/ldv] with kv head g = h / (heads/kv_heads)
 * at [g*dh, (g+1)*dh) -- a KV cache is simply the buffer k/v point into.  Queries are the LAST lens_q[b] positions of
 * the lens_k[b] keys: key j is visible to query i iff j < lens_k[b], (causal) j <= i + lens_k[b] - lens_q[b],
 * (window > 0) j > i + lens_k[b] - lens_q[b] - window.  softmax(scale * q.k) over the visible keys, times v.
 * ------------------------------------------------------------------------------------------ */
enum { MI355_KV_F32 = 0, MI355_KV_BF16 = 1, MI355_KV_F16 = 2 };
typedef struct {
  const float* q; int64_t q_bstride; int32_t ldq;
  const float* k; int64_t k_bstride; int32_t ldk;
  const float* v; int64_t v_bstride; int32_t ldv;
  int32_t heads; int32_t kv_heads; int32_t dh;   /* dh: 64 or 128 */
  int32_t Tq; int32_t Tk;
  const int32_t* lens_q;  /* [B] nullable => Tq */
  const int32_t* lens_k;  /* [B] nullable => Tk */
  int32_t causal; int32_t window; float scale;
  int32_t B;
  int32_t mode;           /* 0 = auto (decode kernel when Tq <= 8), 1 = MFMA flash kernel, 2 = decode kernel */
  float* out; int64_t out_bstride; int32_t ldo;  /* [B, Tq, ldo], head h at [h*dh, (h+1)*dh) */
  const int32_t* k_start; /* [B] nullable: keys j < k_start[b] are left padding (BatchKVCache, lm/models/cache.py:502-560) */
  /* key-range split for decode steps over long key ranges (flash-decoding): partial (max, sum, out) records in split_ws
     [B * heads * Tq * 8 * (dh + 2)] floats, tickets in split_cnt [B * heads * Tq] int32 (zero before the first call; left zero by every call).
     nsplit: 0 = chosen by the library when the workspace is given, 1 = off, 2..8 = forced.  Null workspace = off. */
  float* split_ws; int32_t* split_cnt; int32_t nsplit;
  int64_t k_hstride; int64_t v_hstride; /* 0: kv head g at columns [g*dh, (g+1)*dh) of a row; else head-major planes: head g starts at
                                           g * k_hstride (rows of that head ldk apart, typically ldk = dh) */
  int32_t kv_dtype;       /* element type of k and v: MI355_KV_F32 (0: k / v are float*), MI355_KV_BF16, MI355_KV_F16 (16-bit: the checkpoint dtype the
                             reference keeps its caches in, whisper.py:360-361, lm/models/cache.py:104-176); every k / v stride is in ELEMENTS */
  /* Fused single-query decode step (Tq == 1, causal; talker.py:264-307 q_norm / k_norm / apply_rotary_pos_emb / cache update / sdpa in one launch):
     q holds the RAW projection output; new_k / new_v [B, kv_heads * dh] (items new_bstride floats apart) hold the raw k, v of the new position
     Tk - 1, which is NOT in the cache yet.  The kernel applies the per-head RMSNorm (q_norm_w / k_norm_w [dh], nullable) and the rotary
     embedding (rope_cos / rope_sin [rope_rows, dh / 2], nullable; rope_mode as in mi355_head_rope_args; position rope_pos - k_start[b]) to q and
     to the new k, attends over the cache rows [.., Tk - 1) plus the new pair, and writes the processed k and the v into cache row Tk - 1.
     With lens_k (slot caches of a continuous-batching session) item b's Tk is lens_k[b]: its new row and its rotary position are lens_k[b] - 1. */
  const float* new_k; const float* new_v; int64_t new_bstride;
  const float* q_norm_w; const float* k_norm_w; float norm_eps;
  const float* rope_cos; const float* rope_sin; int32_t rope_rows; int32_t rope_mode; int32_t rope_pos;
  /* the fused step inside the rows pipeline (steps of 9..64 sequences): in_kgroups > 1: q / new_k / new_v point into slab 0 of mi355_rows_gemm's
     partial sums and the kernel adds the in_kgroups slabs (in_kg_stride floats apart, fixed order) plus the projection bias (q_bias [heads dh],
     k_bias / v_bias [kv_heads dh], nullable) itself -- the q | k | v projection needs no separate row epilogue.  out_planes (nullable): the output
     rows additionally (out may then be null) leave as planes of planes_R rows in planes_dtype (MI355_W_BF16 / MI355_W_F16) for the o-proj GEMM;
     item b is row b.  Both need Tq == 1. */
  int32_t in_kgroups; int64_t in_kg_stride; const float* q_bias; const float* k_bias; const float* v_bias;
  const float* q_wscale; const float* k_wscale; const float* v_wscale;   /* nullable: per-column scales of the slab sums (fp8 images), indexed like the biases */
  uint16_t* out_planes; int32_t planes_R; int32_t planes_dtype;
} mi355_flash_attn_args;
int mi355_flash_attention(const mi355_flash_attn_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whisper decode step on device: SuppressBlank -> SuppressTokens -> ApplyTimestampRules -> GreedyDecoder.update
 * (stt/models/whisper/decoding.py:333-443, 302-330), one workgroup per sequence, no host round trip.
 * logits: raw decoder logits of the last position; tokens[b, 0:n] is the context so far (initial tokens included),
 * tokens[b, n] receives the selected token (eot once the sequence has ended), sum_logprobs[b] accumulates
 * log softmax(filtered)[token] while the sequence is alive.  gumbel (nullable): [B, ld] Gumbel(0,1) noise, the
 * explicit-noise form of categorical(logits / temperature) for temperature > 0; null = argmax.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* logits; int32_t ld; int32_t V; int32_t B;
  int32_t* tokens; int32_t tokens_ld; int32_t n;
  int32_t sample_begin;
  const float* suppress_mask;                   /* [V] 0 / -inf, nullable (SuppressTokens) */
  const int32_t* blank_ids; int32_t n_blank;    /* ids masked while n == sample_begin, nullable (SuppressBlank) */
  int32_t timestamp_rules;                      /* 1 = ApplyTimestampRules */
  int32_t timestamp_begin; int32_t eot; int32_t no_timestamps;  /* no_timestamps < 0: tokenizer has none */
  int32_t max_initial_timestamp_index;          /* < 0: None */
  const float* gumbel; float temperature;
  float* sum_logprobs;                          /* [B] */
  float* filtered;                              /* [B, ld] nullable: the filtered logits (parity tests) */
  const int32_t* forced_next;                   /* [B] nullable: teacher forcing -- append this token instead of the selection
                                                   (its log-prob is what gets accumulated) */
  /* optional: spread each row over 16 workgroups (two launches: partial statistics, then filter + selection with the last workgroup of a row
     merging).  split_ws: [B * 16 * 12] floats scratch, split_cnt: [B] int32, zero before the first call and left zero by every call.  Null = one
     workgroup per row. */
  float* split_ws; int32_t* split_cnt;
} mi355_whisper_step_args;
int mi355_whisper_greedy_step(const mi355_whisper_step_args* a, void* stream);
/* out[b] = softmax(logits[b, 0:V])[token]  (no_speech_prob, decoding.py:604-606). */
int mi355_softmax_prob_at(const float* logits, int32_t ld, int32_t V, int32_t B, int32_t token, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Skinny GEMM for decode steps: y[m, n] = epilogue(sum_k x[m, k] * w[n, k]), 1 <= M <= 8 rows.
 * Replaces nn.Linear / Embedding.as_linear at sequence length 1: Whisper TextDecoder (stt/models/whisper/whisper.py:347-416,
 * 498), Qwen3-TTS talker / code predictor (tts/models/qwen3_tts/talker.py:230-330, 503-764), CSM backbone / depth decoder
 * (lm/models/llama.py:46-198, tts/models/sesame/sesame.py:361-404).  HBM-bound: w is read once, row-major [N, ldw] in the
 * checkpoint's 16-bit type (mi355_pack_rowmajor16_host) or as an fp8 image (mi355_pack_rowmajor_fp8_host), products accumulate in fp32.
 * 1..4 rows (and K > 2048 / fp8 at any row count): fp32 FMAs on the exactly decoded weights.  5..8 rows with 16-bit weights and K <= 2048,
 * K % 64 == 0: v_mfma_f32_16x16x32 on the weights' own type with the input rows split into hi + lo images (bf16: ~16 mantissa bits of x, the
 * split the prefill GEMMs use; fp16: ~22) -- environment MI355_GEMV_MFMA=0 keeps the FMA kernel for A/B runs.
 * Epilogue: v = act(acc + bias[n]) * colscale[n] + res[m, n]; y = v * out_scale.  glu = 1: rows of w are interleaved
 * (gate_0, up_0, gate_1, up_1, ...) and y[m, n/2] = silu(acc_gate + b) * (acc_up + b)  (SwiGLU, talker.py TalkerMLP).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* x; int32_t ldx; int32_t M; int32_t K;
  const uint16_t* w; int32_t ldw; int32_t wdtype; int32_t N;   /* wdtype: MI355_W_BF16 / MI355_W_F16 / MI355_W_FP8 (then w holds bytes; ldw in elements) */
  const float* bias;       /* [N] nullable */
  int32_t post_act; float post_slope;
  const float* colscale;   /* [N] nullable */
  const float* res; int32_t ldr;   /* [M, ldr] nullable */
  float out_scale;         /* 0 => 1 */
  int32_t glu;
  float* y; int32_t ldy;
  /* fused input normalisation over K (the pre-LN of a transformer block, whisper.py:407-415 / talker.py:385-396):
     norm = 1: LayerNorm (x - mean) * rsqrt(var + eps) * norm_weight + norm_bias;  norm = 2: RMSNorm x * rsqrt(mean(x^2) + eps) * norm_weight */
  int32_t norm; const float* norm_weight; const float* norm_bias; float norm_eps;
  /* optional second destination: columns n >= split are written to y2[m, n - split] (q -> y, k|v -> the KV-cache slot) */
  float* y2; int32_t ldy2; int32_t split;
  /* MI355_W_FP8 only: per-output-row dequantisation scale [N] (required): acc[n] * wscale[n] precedes the bias */
  const float* wscale;
  int32_t reserved_norm_flag;  /* ignored; callers leave it 0 (kept so the layout of ABI 37 holds) */
  /* optional fused rotary embedding on the first rope_cols output columns (the q | k part of a fused q|k|v projection), interleaved pairs
     (2i, 2i + 1) inside heads of rope_dh channels -- nn.RoPE(traditional=True) / sesame/attention.py:41-105 at ONE position: rope_cos / rope_sin
     point at that position's table row [rope_dh / 2].  Plain epilogue only (no activation / colscale / residual / glu); 1..4 rows. */
  const float* rope_cos; const float* rope_sin; int32_t rope_dh; int32_t rope_cols;
  /* optional gathered input (M == 1 only): the input row is row (x_ids[0] + x_id_offset) of the table x points at (rows ldx floats apart) -- an
     embedding lookup fused into the projection that consumes it (sesame.py:392-396: embed the code just sampled, project it to the decoder width);
     the id is read on the device, so the sampler's output feeds the next GEMV without a host round trip or a separate gather launch */
  const int32_t* x_ids; int32_t x_id_offset;
  float* reserved_ws; int32_t* reserved_cnt;   /* ignored; callers leave them null (kept so the layout of ABI 37 holds) */
  int32_t y2_dtype;   /* element type of y2: MI355_KV_F32 (0) / MI355_KV_BF16 / MI355_KV_F16 -- a 16-bit KV-cache slot (the reference's cache dtype);
                         y2 is then a uint16_t* in disguise and ldy2 counts 16-bit elements */
  int32_t w_policy;   /* cache policy of the weight stream (one-row kernels): 0 = default loads, 1 = non-temporal (`nt`): images that are streamed once
                         per step and should not displace what the step re-reads -- a 2.4 GB backbone in front of a 220 MB depth decoder that runs
                         31 times per frame and fits the 256 MB Infinity Cache (sesame.py:361-404) */
  /* optional attention PROLOGUE (M == 1, K = attn_heads * attn_dh <= 2048, attn_Tk <= 64 cached positions): x is the step's query row (rotated,
     head-major) and the row that enters the product is softmax(q K^T * attn_scale) V over the cache rows 0 .. attn_Tk - 1 (the step's own k | v
     already filed by the q|k|v launch) -- mx.fast.scaled_dot_product_attention + o_proj of lm/models/llama.py:80-96 at one position, one launch
     instead of two where the context is short (CSM's depth decoder: <= 32 positions, sesame.py:385-404).  attn_k / attn_v: row t of kv head g at
     element t * attn_ld + g * attn_dh, element type attn_kv_dtype (MI355_KV_*).  No fused norm / glu / rope / gathered input. */
  const void* attn_k; const void* attn_v; int32_t attn_ld; int32_t attn_Tk; int32_t attn_heads; int32_t attn_kv_heads; int32_t attn_dh;
  float attn_scale; int32_t attn_kv_dtype;
} mi355_gemv_args;
int mi355_gemv(const mi355_gemv_args* a, void* stream);
int mi355_pack_rowmajor16_host(const float* w_host, int64_t n, int32_t dtype, uint16_t* out_host);
/* fp8 weight image for the decode-step GEMVs (BASELINE config[4] names fp8: at <= 8 rows per step a Linear is a weight stream, so the 8-bit
 * image halves the bytes of a step).  Per output row: scale = 2^ceil(log2(max|w| / 448)) (a power of two: the dequantised value
 * q * scale is exactly representable in bf16, so the prefill GEMMs run the SAME quantised weights through the bf16 MFMA image), q = OCP e4m3fn
 * (round-to-nearest-even, max 448).  out_host: rows * cols bytes, scale_host: rows floats; cols % 16 == 0. */
int mi355_pack_rowmajor_fp8_host(const float* w_host, int64_t rows, int64_t cols, uint8_t* out_host, float* scale_host);

/* ------------------------------------------------------------------------------------------
 * Row-wise glue of the decoder-only transformer blocks (Qwen3-TTS talker / code predictor / codec transformer, CSM,
 * Mimi); see mlx_audio_amd/csrc/transformer.hip for the reference call sites of each.
 * ------------------------------------------------------------------------------------------ */
/* nn.RMSNorm over the channel axis: y = x * rsqrt(mean(x^2) + eps) * weight (talker.py:366-369, llama.py:100-104). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;
  int32_t C; int32_t L; const int32_t* lens; int32_t B;
  const float* weight;   /* [C] nullable */
  float eps;
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_rmsnorm_args;
int mi355_rmsnorm(const mi355_rmsnorm_args* a, void* stream);

/* Per-head RMSNorm (q_norm / k_norm, talker.py:264-266) fused with the rotary embedding, out of place: x [B, L, ldx] holds
 * `heads` heads of dh (64 or 128) channels from column 0; y may be a KV-cache slot.  Angles come from host tables
 * cos/sin [rope_rows, dh/2]; position of row l = (pos ? pos[b*pos_ld + l] : pos0 + l) - (pos_sub ? pos_sub[b] : 0).  rope_mode 0 = rotate-half pairs
 * (i, i + dh/2) (talker.py:14-36), 1 = interleaved pairs (2i, 2i+1) (nn.RoPE(traditional=True), sesame/attention.py:41-105). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;
  int32_t heads; int32_t dh; int32_t L; const int32_t* lens; int32_t B;
  const float* norm_weight; float eps;          /* [dh] nullable: no norm */
  const float* cos_table; const float* sin_table; /* nullable: no rotation */
  const int32_t* pos; int32_t pos_ld; int32_t pos0;
  const int32_t* pos_sub;  /* [B] nullable: subtracted from the row's position (left padding of a BatchKVCache row: its first real token is position 0) */
  int32_t rope_rows;       /* rows of cos_table / sin_table; positions are checked (pos0 + L <= rope_rows) or, for device-side positions, clamped */
  int32_t rope_mode;
  float* y; int64_t y_bstride; int32_t ldy;
  /* optional second tensor handled by the same launch with the same positions (q heads -> y, k heads -> the KV-cache slot y2) */
  const float* x2; int64_t x2_bstride; int32_t ldx2; int32_t heads2; const float* norm_weight2;
  float* y2; int64_t y2_bstride; int32_t ldy2;
} mi355_head_rope_args;
int mi355_head_norm_rope(const mi355_head_rope_args* a, void* stream);

/* y[r, i] = silu(x[r, 2i]) * x[r, 2i+1]  (SwiGLU on interleaved gate / up columns, talker.py:312-330). */
int mi355_swiglu(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int32_t I, void* stream);

/* y[b, l, :] = scale * (add[b, l, :] + sum_q table[slot_offset[q] + ids[b, l, q], :]); ids < 0 skip the slot.
 * Codec-embedding sums (qwen3_tts.py:985-1015, sesame.py:361-404) and RVQ decode (codec/models/mimi/modules/quantization.py:
 * 187-191, speech_tokenizer.py:786-800).  ids element (b, l, q) lives at ids + b*ids_bstride + l*ids_ld + q*ids_qstride. */
typedef struct {
  const float* table; int32_t ld_table;
  const int32_t* slot_offset;   /* [Q] row offset of slot q's table inside `table`, nullable => 0 */
  const int32_t* ids; int64_t ids_bstride; int32_t ids_ld; int32_t ids_qstride; int32_t Q;
  const float* add; int64_t add_bstride; int32_t add_ld;   /* nullable */
  float scale;                  /* 0 => 1 */
  int32_t C; int32_t L; const int32_t* lens; int32_t B;
  float* y; int64_t y_bstride; int32_t ldy;
} mi355_embed_sum_args;
int mi355_embed_sum(const mi355_embed_sum_args* a, void* stream);

/* Depthwise conv1d (transpose = 0: y[n] = b + sum_k w[c,k] x[n + k - pad]) or depthwise conv_transpose1d (transpose = 1:
 * y[n] = b + sum over t*stride + k - pad == n of w[c,k] x[t]), channels-last, zero outside [0, lens_in[b]).
 * `stride` belongs to the transposed conv alone: the plain conv has none, and transpose = 0 with stride > 1 is refused.
 * ConvNeXt dwconv k7 of the Qwen3 codec decoder (speech_tokenizer.py ConvNeXtBlock), Mimi's depthwise upsampler (mimi.py:296-320),
 * SNAC's depthwise convs (codec/models/snac/layers.py:170-181, 209-233). */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx; int32_t Lin; const int32_t* lens_in;
  const float* w;      /* [C, K] */
  const float* bias;   /* [C] nullable */
  int32_t C; int32_t K; int32_t pad; int32_t stride; int32_t transpose; int32_t B;
  float* y; int64_t y_bstride; int32_t ldy; int32_t Lout;
  /* transpose = 0 only: dilation (0 => 1; tap k reads x[n + k * dil - pad]) and an optional Snake prologue per channel,
     x -> x + pre_inv[c] * sin(pre_alpha[c] * x)^2 -- the depthwise k7 of SNAC's ResidualUnit (codec/models/snac/layers.py:209-233, 298-306) */
  int32_t dil; const float* pre_alpha; const float* pre_inv;
} mi355_dwconv_args;
int mi355_dwconv(const mi355_dwconv_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Token sampling for the codec-token LMs: suppress -> repetition penalty -> / temperature -> top-k -> top-p / min-p ->
 * categorical (Gumbel-max on caller-supplied noise).  Replaces Model._sample_token(_batch) (tts/models/qwen3_tts/qwen3_tts.py:
 * 805-925) and lm/sample_utils.py:130-281.  One workgroup per row, V <= 8192.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* logits; int32_t ld; int32_t V; int32_t B;
  const float* suppress_mask;     /* [V] 0 / -inf, nullable */
  const int32_t* history; int32_t hist_ld; int32_t n_hist; const int32_t* hist_len;  /* generated tokens [B, hist_ld]; per-row count
                                                                                        hist_len[b] (nullable => n_hist) */
  float repetition_penalty;       /* 1 = off */
  float temperature;              /* <= 0: arg-max of the penalised logits */
  int32_t top_k;                  /* <= 0 or >= V: off */
  float top_p; float min_p;       /* top_p outside (0, 1): off; min_p = 0: off */
  const float* gumbel;            /* [B, ld] Gumbel(0,1) noise, nullable => arg-max */
  const int32_t* done; int32_t done_token;  /* nullable: rows with done[b] != 0 emit done_token */
  int32_t* out; int32_t out_ld;   /* token of row b -> out[b * out_ld] */
  float* filtered;                /* [B, ld] nullable: logits after all filters (parity tests) */
} mi355_sample_args;
int mi355_sample(const mi355_sample_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Native decode-step runner: one call launches every kernel of a single-position step of a whole decoder stack (<= 64 sequences; 9..64 run
 * the rows pipeline -- mi355_rows_gemm / mi355_rows_finish -- on the tile images of the layer records),
 * replacing the per-op Python schedule of TalkerDecoderLayer / Qwen3TTSTalkerModel.__call__ (tts/models/qwen3_tts/talker.py:385-500),
 * CodePredictorModel (talker.py:615-690), LlamaModel (lm/models/llama.py:160-198) and Whisper's TextDecoder blocks with self- and
 * cross-attention (stt/models/whisper/whisper.py:405-416, 476-498).  All weights are row-major 16-bit images (mi355_pack_rowmajor16_host);
 * the KV cache of layer i is kv [B, kv_capacity, 2*kv_heads*dh] fp32 (k columns, then v), row `offset` is written by the step.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const uint16_t* wqkv; const float* bqkv;      /* [(heads + 2 kv_heads) dh, d_model]: q | k | v rows */
  const uint16_t* wo; const float* bo;          /* [d_model, heads dh] */
  const uint16_t* w_in; const float* b_in;      /* SwiGLU: [2 d_ff, d_model] with gate / up rows interleaved; else [d_ff, d_model] */
  const uint16_t* w_out; const float* b_out;    /* [d_model, d_ff] */
  const float* attn_norm_w; const float* attn_norm_b; const float* mlp_norm_w; const float* mlp_norm_b;
  const float* q_norm; const float* k_norm;     /* [dh] per-head RMSNorm weights, nullable */
  const float* ls1; const float* ls2;           /* [d_model] LayerScale, nullable */
  float* kv; int64_t kv_bstride; int32_t kv_capacity;   /* element type = mi355_stack_desc.kv_dtype (then kv is a uint16_t* in disguise); strides in elements */
  /* optional cross-attention block (Whisper decoder): q projection + pre-norm, K | V precomputed [B, cross_len, 2*kv_heads*dh] */
  const uint16_t* wcq; const float* bcq; const uint16_t* wco; const float* bco;
  const float* cross_norm_w; const float* cross_norm_b;
  const float* cross_k; const float* cross_v;   /* head-major [B, kv_heads, cross_len, dh] each (a head's keys contiguous) */
  int64_t cross_bstride; int64_t cross_hstride; int32_t cross_ld; int32_t cross_len;
  int32_t cross_kv_dtype;   /* MI355_KV_F32 / MI355_KV_BF16 / MI355_KV_F16: element type of cross_k / cross_v (strides in elements) */
  /* wdtype == MI355_W_FP8: per-row scales of the six images (mi355_pack_rowmajor_fp8_host), else null */
  const float* s_qkv; const float* s_o; const float* s_in; const float* s_out; const float* s_cq; const float* s_co;
  /* steps for 9..64 sequences: tile images (mi355_pack_tiles16_host) of the four projections; null = this layer only runs steps of <= 8 sequences */
  const uint16_t* wqkv_t; const uint16_t* wo_t; const uint16_t* w_in_t; const uint16_t* w_out_t;
  const uint16_t* wcq_t; const uint16_t* wco_t;   /* ... and of the cross-attention projections (Whisper decoder at 9..64 windows per step) */
} mi355_layer_desc;

typedef struct {
  int32_t n_layers; int32_t d_model; int32_t heads; int32_t kv_heads; int32_t dh; int32_t d_ff;
  int32_t norm;            /* 1 = LayerNorm, 2 = RMSNorm */
  float eps;
  int32_t glu;             /* 1 = SwiGLU MLP */
  int32_t act;             /* MLP activation when glu == 0 (MI355_ACT_GELU, MI355_ACT_GELU_TANH, ...) */
  int32_t wdtype;          /* MI355_W_BF16 / MI355_W_F16 / MI355_W_FP8 (every image of the stack, scales in the layer records) */
  int32_t causal; int32_t window;
  float attn_scale;        /* 0 => dh^-0.5 */
  int32_t rope_mode; const float* cos; const float* sin;   /* tables [rope_rows, dh/2], nullable: no rotary embedding */
  int32_t rope_rows;       /* table rows: a step at offset >= rope_rows is refused (sesame.py:817-820 raises for the same reason) */
  const int32_t* k_start;  /* [B] nullable: left padding of each sequence (lm/models/cache.py:502-560 BatchKVCache): keys before it are invisible,
                              RoPE positions count from it */
  const mi355_layer_desc* layers;                           /* HOST array of n_layers records */
  float* attn_split_ws; int32_t* attn_split_cnt;            /* nullable: workspace of mi355_flash_attn_args.split_* for B <= 8, Tq = 1 */
  float* reserved_gemv_ws; int32_t* reserved_gemv_cnt;      /* ignored; callers leave them null (kept so the layout of ABI 37 holds) */
  const float* final_norm_w; const float* final_norm_b;     /* nullable */
  int32_t kv_dtype;        /* MI355_KV_F32 / MI355_KV_BF16 / MI355_KV_F16: element type of every layer's kv buffer (the reference keeps its caches in the
                              checkpoint dtype, lm/models/cache.py:104-176).  16-bit caches need the stores that exist: q|k|v GEMV with the rotary pairs in its
                              epilogue, the fused norm / rope attention step, or no rotary embedding at all */
  void* rows_ws; int64_t rows_ws_bytes;   /* steps for 9..64 sequences: planes + partial slabs, mi355_stack_rows_ws_bytes(d, B) bytes (nullable otherwise) */
  const int32_t* slot_lens_k;  /* [B] nullable (device): SLOT caches of a continuous-batching session -- sequence b holds slot_lens_k[b] - 1 cached positions
                                  and this step appends position slot_lens_k[b] - 1 to ITS row of every kv buffer (rotary position = that index); `offset`
                                  is then only the host's upper bound of the positions (capacity / table checks).  Needs the fused attention step
                                  (per-head norms and / or rotary embedding, causal). */
  int32_t w_policy;        /* mi355_gemv_args.w_policy of every projection of the stack (steps of 1 sequence) */
} mi355_stack_desc;

/* ------------------------------------------------------------------------------------------
 * Unidirectional LSTM over a whole sequence, any hidden size (EnCodec's two 512-wide layers, codec/models/encodec/encodec.py:89-167: the
 * reference's Metal `lstm` kernel + one matmul per step).  xproj [B, T, 4H] = x @ Wx^T + bias for all steps (the caller's GEMM), gate chunks in the
 * order i | f | g | o; wh: row-major 16-bit image [4H, H] (mi355_pack_rowmajor16_host); h, c [B, H] fp32 state (in: initial, normally zeros; out:
 * final); pre [B, 4H] scratch; out [B, T, H].  Two launches per time step (mi355_gemv with the x-projection row as residual, then the gates) --
 * or ONE (round 5, ABI 32): with gate_interleaved = 1 the rows of `wh` are ordered by hidden unit (row 4 j + g = gate g of unit j instead of the
 * reference's g H + j), so a 16-row tile of the step's GEMM holds all four gates of four units and the gates, the cell update and the stores of h
 * are that GEMM's epilogue; h then ping-pongs between `h` and the scratch `h2` (every workgroup reads the whole previous h), the final state ends
 * up in `h`.  Needs H % 64 == 0; `pre` is not used.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* xproj; int64_t xproj_bstride; int32_t ld_xproj;
  const uint16_t* wh; int32_t wdtype;   /* MI355_W_BF16 / MI355_W_F16 */
  float* h; float* c; float* pre;
  float* out; int64_t out_bstride; int32_t ld_out;
  int32_t B; int32_t T; int32_t H;
  int32_t gate_interleaved;   /* 0: wh rows in the reference's i | f | g | o blocks (two launches per step); 1: row 4 j + g (one launch per step) */
  float* h2;                  /* [B, H] scratch, gate_interleaved = 1 only */
} mi355_lstm_seq_args;
int mi355_lstm_seq(const mi355_lstm_seq_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decode steps for a batch of 9..64 sequences (BASELINE config[3]: 64 utterances; the reference's batched generation
 * tts/models/qwen3_tts/qwen3_tts.py:1651-2060 over talker.py:229-336, 385-500): nn.Linear at sequence length 1 as
 *   mi355_rows_gemm   (pure matrix-pipe GEMM: tile image of W x pre-split input planes -> fp32 partial slabs, one per K group)
 *   mi355_rows_finish (row epilogue: sum of the slabs in a fixed order, then the epilogue of mi355_gemv, optional normalisation of the
 *                      finished row, optional output as planes for the next mi355_rows_gemm; kgroups = 1: converter fp32 rows -> planes).
 * Planes: the input rows as hi + lo images of the weights' 16-bit type (x ~= hi + lo: ~16 mantissa bits for bf16, ~22 for fp16) in MFMA fragment
 * order: 16-byte piece ((((s * 2 + image) * 2 + half) * 4 + group) * R + row) holds x[row][64 s + 16 group + 8 half .. + 8), R = 16 / 32 / 64 rows;
 * 4 * R * K bytes for K columns.  Rows >= M of the planes are never read into a stored result.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const uint16_t* wt;       /* tile image of W [N, K] from mi355_pack_tiles16_host (MI355_W_FP8: the byte image of mi355_pack_tiles8_host) */
  int32_t wdtype;           /* MI355_W_BF16 / MI355_W_F16 (planes must hold the same type) / MI355_W_FP8 (OCP e4m3fn bytes, decoded to bf16 in registers: exact;
                               planes hold bf16; the per-row scales are applied by the row epilogue: mi355_rows_finish_args.wscale) */
  int32_t N; int32_t K;     /* K % 64 == 0 */
  const uint16_t* planes;   /* the input rows (written by mi355_rows_finish) */
  int32_t M; int32_t R;     /* rows in use / rows of the planes (16, 32 or 64) */
  float* part;              /* slab g at part + g * kg_stride: [M, ldp] fp32 partial sums over the g-th range of k steps */
  int32_t ldp; int64_t kg_stride;
  int32_t kgroups;          /* mi355_rows_kgroups(N, K) (or any count that leaves no K group empty) */
  /* kgroups == 1 only (a workgroup then holds complete sums): fused SwiGLU epilogue -- columns are (gate, up) pairs, planes_out receives
     silu(gate + bias) * (up + bias) [M, N / 2] as planes of R rows (N % 128 == 0), nothing is written to part (which may then be null) */
  uint16_t* glu_planes_out; const float* glu_bias;
  const float* wscale;      /* fused SwiGLU epilogue of an fp8 image only: per-row scales [N] (applied to the sums before the bias) */
} mi355_rows_gemm_args;
int mi355_rows_gemm(const mi355_rows_gemm_args* a, void* stream);
int32_t mi355_rows_kgroups(int32_t N, int32_t K);
/* fp32 [N, K] (host) -> tile image: element e of (tile t, k step s, group g, row i) = W[16 t + i][64 s + 16 g + e], stored
 * [ceil(N / 16)][K / 64][4][16][16]; rows past N are zero.  out: ceil(N / 16) * 16 * K 16-bit elements.  dtype: MI355_W_BF16 / MI355_W_F16 */
int mi355_pack_tiles16_host(const float* w_host, int64_t N, int64_t K, int32_t dtype, uint16_t* out_host);
/* uint8 [N, K] e4m3 codes (mi355_pack_rowmajor_fp8_host) -> the fp8 tile image, same order, one byte per element; out: ceil(N / 16) * 16 * K bytes */
int mi355_pack_tiles8_host(const uint8_t* codes_host, int64_t N, int64_t K, uint8_t* out_host);

typedef struct {
  const float* part; int32_t kgroups; int64_t kg_stride; int32_t ldp;   /* input: sum over g of part[g * kg_stride + m * ldp + n]; kgroups = 1: a plain fp32 matrix */
  int32_t M; int32_t N;
  /* epilogue of mi355_gemv: v = act(sum + bias[n]) * colscale[n] + res[m, n]; v *= out_scale;  glu = 1: columns are (gate, up) pairs and
     v[m, n / 2] = silu(gate + b) * (up + b) * out_scale */
  const float* bias; int32_t post_act; float post_slope; const float* colscale; const float* res; int32_t ldr; float out_scale; int32_t glu;
  const float* wscale;      /* nullable: per-column scale of the SUM, before the bias (the per-row dequantisation scales of an fp8 image) */
  float* y; int32_t ldy;    /* nullable: the finished row as fp32 (may alias res) */
  float* y2; int32_t ldy2; int32_t split; int32_t y2_dtype;   /* nullable: columns >= split go to y2[m, n - split] (the KV-cache slot, MI355_KV_*) */
  /* optional normalisation of the finished row over its N (glu: N / 2) outputs, feeding yn / planes: 1 = LayerNorm, 2 = RMSNorm */
  int32_t norm; const float* norm_weight; const float* norm_bias; float norm_eps;
  float* yn; int32_t ldyn;  /* nullable: the (normalised) row as fp32 (a stack's final norm) */
  uint16_t* planes; int32_t R; int32_t planes_dtype;   /* nullable: the (normalised) row as planes of R rows in MI355_W_BF16 / MI355_W_F16 (row length % 64 == 0) */
} mi355_rows_finish_args;
int mi355_rows_finish(const mi355_rows_finish_args* a, void* stream);

/* x [B, d_model] (updated in place: the residual stream), ws: workspace of B * (2 * heads * dh + d_ff + 2 * kv_heads * dh) floats, out (nullable) [B, d_model]
 * receives the final-normed hidden state when final_norm_w is set.  offset = rows already in the KV caches. */
int mi355_stack_decode_step(const mi355_stack_desc* d, float* x, int32_t B, int32_t offset, float* ws, float* out, void* stream);
/* bytes of mi355_stack_desc.rows_ws a step of B (9..64) sequences needs (planes of the three GEMM inputs + the largest set of partial slabs) */
int64_t mi355_stack_rows_ws_bytes(const mi355_stack_desc* d, int32_t B);

/* ------------------------------------------------------------------------------------------
 * Whisper word-level timestamps (stt/models/whisper/timing.py:111-181): cross-attention alignment weights, the standardise / median / head-mean
 * matrix and the dynamic-time-warping path, all on the device (align.hip).  Every kernel takes B items with per-item lengths; nothing is read
 * or written beyond an item's own lengths.  The library allocates nothing.
 *
 * mi355_align_qk_softmax: w[b, slot, t, f] = softmax over f of (qk_scale * scale * q[b, t, head] . k[b, f, head]), float32, for the n_pairs
 * (head, slot) pairs of one decoder layer.  q [B, T, ldq] float32, head h at columns [h*dh, (h+1)*dh); k as in mi355_flash_attn_args (rows: head h
 * at element h*dh of a row, rows ldk apart; k_hstride != 0: head-major planes), element type kv_dtype (MI355_KV_*), strides in elements; dh 64 or 128.
 * lens_t / lens_f nullable (then T / F).  w is [B, A, Tmax, Fmax] with the strides given (floats). */
typedef struct {
  const float* q; int64_t q_bstride; int32_t ldq;
  const void* k; int64_t k_bstride; int64_t k_hstride; int32_t ldk; int32_t kv_dtype;
  int32_t dh; int32_t B; int32_t T; int32_t F;
  const int32_t* lens_t; const int32_t* lens_f;
  const int32_t* pairs; int32_t n_pairs;      /* device int32 [n_pairs, 2]: (head, slot) */
  int32_t heads;                              /* heads per q row (validates nothing on the device: every pair's head must be < heads) */
  float scale; float qk_scale;
  float* w; int64_t w_bstride; int64_t w_astride; int32_t ldw; int32_t A;   /* w[b, slot, t, f] at b*w_bstride + slot*w_astride + t*ldw + f; slot < A */
} mi355_align_qk_args;
int mi355_align_qk_softmax(const mi355_align_qk_args* a, void* stream);

/* mi355_align_matrix (timing.py:148-154): per (head, frame) the mean and population standard deviation over the lens_t[b] tokens, (w - mean) / std
 * (IEEE division), a median filter of odd width medfilt_width (<= 15) along the frames with reflect padding (values pass unfiltered when
 * F <= medfilt_width / 2), the mean over the A heads, token rows [row_begin, lens_t[b] - row_trim) kept, and out[b, n, f] = (negate ? -1 : 1) * that.
 * standardize = 0 skips the statistics (a plain median filter when A = 1).  stats: caller's scratch of B * A * F * 2 floats (unused when standardize = 0). */
typedef struct {
  const float* w; int64_t w_bstride; int64_t w_astride; int32_t ldw; int32_t A;
  int32_t B; int32_t T; int32_t F; const int32_t* lens_t; const int32_t* lens_f;
  int32_t medfilt_width; int32_t standardize; int32_t negate; int32_t row_begin; int32_t row_trim;
  float* stats;
  float* out; int64_t out_bstride; int32_t ldo;
} mi355_align_matrix_args;
int mi355_align_matrix(const mi355_align_matrix_args* a, void* stream);

/* mi355_dtw (timing.py:52-99): cost [B, N, ldc] float32 with lens_n[b] x lens_m[b] valid cells per item (nullable: N x M) -> the warping path in forward
 * order, text_idx[b, 0:path_len[b]] / time_idx[b, ...] (int32, items path_cap >= N + M apart).  float32 accumulation, one add per cell, the reference's
 * comparison chain and border handling: given the same input the path is the reference's bit for bit.  N <= 1024.  ws: mi355_dtw_ws_bytes(N, M, B) bytes. */
typedef struct {
  const float* cost; int64_t cost_bstride; int32_t ldc;
  int32_t B; int32_t N; int32_t M; const int32_t* lens_n; const int32_t* lens_m;
  int32_t* text_idx; int32_t* time_idx; int32_t path_cap; int32_t* path_len;
  void* ws; int64_t ws_bytes;
} mi355_dtw_args;
int mi355_dtw(const mi355_dtw_args* a, void* stream);
int64_t mi355_dtw_ws_bytes(int32_t N, int32_t M, int32_t B);

/* out[r] = softmax(logits[r, 0:V])[tokens[r]] with a per-row token id (timing.py:135-139); a token outside [0, V) gives 0 without a read. */
int mi355_softmax_prob_rows(const float* logits, int64_t ld, int32_t V, int32_t R, const int32_t* tokens, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Unidirectional GRU over whole sequences with MLX nn.GRU semantics (the GRU behind SqueezedGRU, sts/models/deepfilternet/network.py:153-192).
 * One entry point added to ABI 37 (new struct and function only; no existing layout changed).  One persistent workgroup per sequence, the
 * recurrent weights resident on the CU (gru.hip).  xproj [B, T, 3H] = x @ Wx^T + b for all steps (the caller's GEMM), gate blocks r | z | n
 * (PyTorch's bias_hh r / z parts folded into b).  With h_{-1} = h0[b] (NULL: zeros), for t < n = lens[b] (NULL: T; clamped to [0, T]):
 *   r = sigmoid(x_r + (Wh h)_r),  z = sigmoid(x_z + (Wh h)_z),  n = tanh(x_n + r * ((Wh h)_n + bhn)),  h = (1 - z) * n + z * h,  out[b, t] = h;
 * output rows n <= t < T are written as zeros; hT[b] (nullable) receives the state after step n (h0[b] when n = 0).
 * wh: IEEE-half image of Wh / wh_scale [3H, H] as 16-byte groups [H / 8][3H][8] (group (kg, row) = Wh[row, 8 kg .. 8 kg + 8)), 16-byte aligned;
 * wh_scale a power of two (0 = 1) that multiplies every recurrent sum (the scheme of mi355_lstm_args.wh_scale).  fp32 accumulation in a fixed
 * order: two calls on the same bytes give the same bits.  H 64, 128 or 256; MI355_ERR_UNSUPPORTED without a launch for any other H.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* xproj; int64_t xproj_bstride; int32_t ld_xproj;   /* [B, T, ld_xproj], ld_xproj >= 3H */
  const uint16_t* wh; float wh_scale;
  const float* bhn;                                              /* [H] */
  const float* h0;                                               /* [B, H] nullable => zeros */
  const int32_t* lens;                                           /* [B] nullable => T */
  int32_t B; int32_t T; int32_t H;
  float* out; int64_t out_bstride; int32_t ld_out;               /* [B, T, ld_out], ld_out >= H */
  float* hT;                                                     /* [B, H] nullable */
} mi355_gru_seq_args;
int mi355_gru_seq(const mi355_gru_seq_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * DeepFilterNet2 / 3 (sts/models/deepfilternet): the feature front end, the fused conv block and the mask + deep-filter back end (dfn.hip).
 * Three entry points added to ABI 37 (new structs and functions only).  Plain float32 in the reference's operation order (no contraction), every
 * output element a fixed sum: two calls on the same bytes give the same bits.  Spectra are interleaved (re, im) float pairs [B, T, F, 2]; the
 * activations are channels-last [B, T, F, C] and contiguous behind their batch stride.  lens [B] nullable (then T), clamped to [0, T].
 * ------------------------------------------------------------------------------------------ */
#define MI355_DFN_MAX_BANDS 256   /* nb_erb and nb_df of mi355_dfn_features */
#define MI355_DFN_MAX_CH 64       /* channels on either side of mi355_dfn_conv2d */
/* model.py:306-323,366-410 + DfNet._apply_lookahead (network.py:759-773).  spec_out = spec * wnorm (all F bins); per frame the ERB energies of
 * |spec_out|^2 -- erb_fb [F, E] given: the filterbank product; NULL: the mean over band e's bins [erb_start[e], erb_start[e + 1]) --, then
 * 10 log10(. + 1e-10) and the two running normalisations  state = x * one_minus_alpha + state * alpha  (states start at linspace(-60, -90, E) and
 * linspace(0.001, 0.0001, D), x = the dB value / |spec_out| of bin d < D): erb = (x - state) / 40, df = spec_out / sqrt(state).  With n = lens[b]:
 * feat[t] = norm[t + la] for t + la < n, zeros for the rest of [0, T) (la = lookahead if n > lookahead else 0: the reference skips the shift).
 * Two launches: the band energies per (frame, item) in parallel (the dB values pass through feat_erb), then the two recurrences, one thread per
 * band / bin, sequential over the item's frames.  E, D <= MI355_DFN_MAX_BANDS, D <= F. */
typedef struct {
  const float* spec; int64_t spec_bstride;            /* [B, T, F, 2] */
  float wnorm; float alpha; float one_minus_alpha;
  const float* erb_fb; const int32_t* erb_start;      /* [F, E] or [E + 1] (device); exactly one is given */
  const int32_t* lens; int32_t B; int32_t T; int32_t F; int32_t E; int32_t D; int32_t lookahead;
  float* spec_out; int64_t spec_out_bstride;          /* [B, T, F, 2] (may alias spec) */
  float* feat_erb; float* feat_df;                    /* [B, T, E] and [B, T, D, 2], contiguous */
} mi355_dfn_features_args;
int mi355_dfn_features(const mi355_dfn_features_args* a, void* stream);

/* The fused conv block (network.py:249-319,357-417,478-556,559-649), x [B, T, F, Cin] -> y [B, T, Fo, Cout]:
 *   mid = conv(x) with w in the PyTorch layout -- [Cmid, Cin / groups, kt, kf] (Conv2d) or, transposed = 1, [Cin, Cmid / groups, kt, kf]
 *         (ConvTranspose2d), kt <= 5, kf 1 or 3; time: kt - 1 - lookahead zero frames on the left, lookahead on the right, frames at and beyond
 *         lens[b] read as zero (transposed: padding kt - 1, i.e. frame t + kt - 1 - k under tap k); frequency: padding kf / 2 at fstride 1 or 2
 *         (Fo = (F + 2 (kf / 2) - kf) / fstride + 1), or transposed at stride fstride with padding kf / 2 and output padding kf / 2
 *         (Fo = (F - 1) fstride + kf - kf / 2);
 *   v   = pw [Cout, Cmid] @ mid when pw is given (else Cout = Cmid, v = mid);
 *   y   = act(v * scale[c] + shift[c]) + add   (scale / shift: the folded BatchNorm, nullable => 1 / 0; act 0 none, 1 ReLU, 2 sigmoid;
 *         add [B, T, Fo, Cout] nullable, added AFTER the activation).
 * Output frames at and beyond lens[b] are zeros.  One read of x and one write of y. */
typedef struct {
  const float* x; int64_t x_bstride;
  const float* w; const float* pw; const float* scale; const float* shift;
  const float* add; int64_t add_bstride;
  const int32_t* lens;
  int32_t B; int32_t T; int32_t F; int32_t Cin; int32_t Cmid; int32_t Cout; int32_t groups;
  int32_t kt; int32_t kf; int32_t lookahead; int32_t fstride; int32_t transposed; int32_t act;
  float* y; int64_t y_bstride;
} mi355_dfn_conv2d_args;
int mi355_dfn_conv2d(const mi355_dfn_conv2d_args* a, void* stream);
int32_t mi355_dfn_conv2d_fo(int32_t F, int32_t kf, int32_t fstride, int32_t transposed);

/* Mask, deep filter and assembly (network.py:671-736,786-804; model.py:329-333).  gain[t, f] = sum_e m[b, t, e] erb_inv_fb[e, f];
 * df[t, f] = sum_k S[t + k - (order - 1 - df_lookahead), f] * coef[b, t, f, k] (complex; frames outside [0, lens[b]) are zero) for f < D, where
 * S = spec * gain when mask_first = 1 (enc_concat: the filter sees the masked spectrum) and S = spec otherwise;
 * out = (f < D ? df : spec * gain) / wnorm; frames at and beyond lens[b] are zeros. */
typedef struct {
  const float* spec; int64_t spec_bstride;            /* [B, T, F, 2] */
  const float* m; const float* erb_inv_fb;            /* [B, T, E] contiguous; [E, F] */
  const float* coef;                                  /* [B, T, D, order, 2] contiguous */
  const int32_t* lens; int32_t B; int32_t T; int32_t F; int32_t E; int32_t D; int32_t order; int32_t df_lookahead; int32_t mask_first;
  float wnorm;
  float* out; int64_t out_bstride;                    /* [B, T, F, 2] */
} mi355_dfn_apply_args;
int mi355_dfn_apply(const mi355_dfn_apply_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mel-Band RoFormer (sts/models/mel_roformer): the ragged band split, the ragged band merge and the per-head sigmoid gate (bandsplit.hip).
 * Three entry points added to ABI 37 (new structs and functions only).  Plain float32, no atomics, nothing allocated; every output element is
 * a sum in a fixed order that does not depend on the launch geometry: two calls on the same bytes give the same bits.
 *
 * Spectra are the output of mi355_stft for the B * 2 channel items: item b, channel c, frame t, bin f at spec + (2 b + c) * spec_cstride +
 * t * spec_tstride + 2 f (re, im).  A CaC index is j = 2 * bin + channel, 0 <= j < 2 F.  The band tables are CSR lists of CaC indices built on
 * the host: band n owns band_idx[band_ptr[n] .. band_ptr[n + 1]) -- any indices in any order (no contiguity, no limit on how many bands share an
 * index) -- and its vector u has bd_n = 2 * (band_ptr[n + 1] - band_ptr[n]) entries: u[2 m] = Re, u[2 m + 1] = Im of its m-th index.  A table
 * index outside [0, 2 F) reads as zero.  No pointer needs more than float alignment.
 * ------------------------------------------------------------------------------------------ */
#define MI355_BAND_MAX_DIM 960    /* largest bd_n of mi355_band_split: 16 frames of a band stay in 60 KiB of LDS */
/* BandSplit.split (mel_roformer/model.py:299-336) with the RMSNorm of model.py:26-42:
 *   y[b, t, n, :] = W_n (u / max(||u||_2, 1e-12) * sqrt(bd_n) * gamma_n) + bias_n,   y [B, T, Nb, D] contiguous behind y_bstride.
 * An all-zero frame gives exactly bias_n.  wt: the ragged concatenation of the TRANSPOSED weights, band n's [bd_n, D] block at wt + D * 2 *
 * band_ptr[n]; gamma: ragged, band n at gamma + 2 * band_ptr[n]; bias [Nb, D].  One workgroup per (band, 16 frames, item): the normalised frames
 * wait in LDS and each weight is read once per workgroup.  ||u||^2 is summed by one wave per frame (lane l adds entries l, l + 64, ... in order,
 * then the xor butterfly); each output is a sequential sum over the band's entries.  max_band_dim: the largest bd_n of the table (the host
 * built it), at most MI355_BAND_MAX_DIM, else MI355_ERR_UNSUPPORTED without a launch; a band wider than declared is left unwritten. */
typedef struct {
  const float* spec; int64_t spec_cstride; int64_t spec_tstride;
  const int32_t* band_ptr; const int32_t* band_idx; int32_t n_idx;   /* [Nb + 1], [n_idx] (device); n_idx = band_ptr[Nb] */
  int32_t max_band_dim;
  const float* wt; const float* gamma; const float* bias;
  int32_t B; int32_t T; int32_t F; int32_t Nb; int32_t D;
  float* y; int64_t y_bstride;
} mi355_band_split_args;
int mi355_band_split(const mi355_band_split_args* a, void* stream);

/* MaskEstimator's GLU, BandSplit.merge and the complex product (model.py:338-368,419-421,623-634) as one gather.  h [B, T, h_cols] (row t of
 * item b at h + b * h_bstride + t * ldh) is the last per-band Linear's output, band n at columns [4 band_ptr[n], 4 band_ptr[n + 1]): bd_n values,
 * then bd_n gates.  The host inverts the band tables: CaC index j lists its contributors inv_col / inv_bd [inv_ptr[j] .. inv_ptr[j + 1]) in
 * ascending band order (the reference's addition order): col = the column of the contributor's real part (the imaginary part at col + 1), bd =
 * that band's bd_n (the gates bd columns further).  A contributor whose columns leave [0, h_cols) is skipped.
 *   mask[j] = (sum_c h[col_c + {0, 1}] * sigmoid(h[col_c + bd_c + {0, 1}])) / max(count_j, 1)   (complex; an index nobody covers has mask 0)
 *   out[2 b + c, f, t] = spec[2 b + c, t, f] * mask[2 f + c]                                   (complex)
 * at out + (2 b + c) * out_cstride + f * out_fstride + t * out_tstride (+ 0 / 1 for re / im; strides in floats): [B * 2, F, T] as
 * mlx_audio.dsp.istft takes it, or any other order.  One thread per (item, frame, CaC index). */
typedef struct {
  const float* h; int64_t h_bstride; int64_t ldh; int32_t h_cols;
  const int32_t* inv_ptr; const int32_t* inv_col; const int32_t* inv_bd; int32_t n_inv;   /* [2 F + 1], [n_inv], [n_inv] (device); n_inv = inv_ptr[2 F] */
  const float* spec; int64_t spec_cstride; int64_t spec_tstride;
  int32_t B; int32_t T; int32_t F;
  float* out; int64_t out_cstride; int64_t out_fstride; int64_t out_tstride;
} mi355_band_merge_args;
int mi355_band_merge(const mi355_band_merge_args* a, void* stream);

/* RoFormerAttention's gate (model.py:237-239), in place on channels-last views: x[b, l, h * dh + i] *= sigmoid(g[b, l, h]) for h < heads,
 * i < dh; x [B, L, ldx >= heads * dh], g [B, L, ldg >= heads] (e.g. the columns behind q | k | v of one projection). */
typedef struct {
  float* x; int64_t x_bstride; int64_t ldx;
  const float* g; int64_t g_bstride; int64_t ldg;
  int32_t heads; int32_t dh; int32_t L; int32_t B;
} mi355_head_gate_args;
int mi355_head_gate(const mi355_head_gate_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * SenseVoice-Small (stt/models/sensevoice/sensevoice.py): the encoder's input assembly and the CTC head behind the ctc_lo GEMM (sanm.hip).
 * Three entry points added to ABI 37 (new structs and functions only; no existing layout changed).  Plain float32, no atomics, nothing
 * allocated; every output is computed in a fixed order that does not depend on the launch geometry: two calls on the same bytes give the
 * same bits.  (The SAN-M memory term itself is mi355_fsmn_memory.)
 * ------------------------------------------------------------------------------------------ */
/* _apply_lfr + _apply_cmvn (sensevoice.py:47-80), the query rows of SenseVoiceSmall.__call__ (:426-433) and the encoder's scale and
 * SinusoidalPositionEncoder (:106-122,322-324) in one launch.  With W = lfr_m * D, left = (lfr_m - 1) / 2, n_b = lens[b] (NULL: T) and
 * R_b = 4 + ceil(n_b / lfr_n), the output x [B, 4 + ceil(T / lfr_n), W] is
 *   row r < 4:           u = embed[qids[b, r]]
 *   row 4 + i < R_b:     u[j * D + d] = feats[b, clamp(i * lfr_n + j - left, 0, n_b - 1), d]   (j < lfr_m: left-padded with frame 0, right-padded
 *                        with the ITEM's last valid frame, not with row T - 1 of the batch), then u = (u + means) * istd when means / istd are given
 *   every row r < R_b:   x[b, r] = u * scale + pe[r]     (each operation rounded on its own, in this order; pe NULL: no position term)
 *   rows r >= R_b:       zeros
 * and out_lens[b] = R_b.  pe [pe_rows >= 4 + ceil(T / lfr_n), W] is the host's sinusoidal table (positions from 1, sines in the first half of
 * the columns, cosines in the second).  qids in [0, 16).  1 <= lens[b] <= T is the caller's contract (an item without a frame has no last
 * frame to pad with); the kernel clamps what it reads so that no index leaves feats.  lfr_m = lfr_n = 1 passes already stacked features. */
typedef struct {
  const float* feats; int64_t feats_bstride; int32_t ldf;  /* [B, T, ldf], ldf >= D */
  const int32_t* lens;                                     /* [B] nullable => T */
  const float* means; const float* istd;                   /* [W] nullable (together) */
  const float* embed; const int32_t* qids;                 /* [16, W]; [B, 4] */
  const float* pe; int32_t pe_rows;                        /* [pe_rows, W] nullable */
  int32_t lfr_m; int32_t lfr_n; float scale;
  int32_t B; int32_t T; int32_t D;
  float* x; int64_t x_bstride; int32_t ldx;                /* [B, 4 + ceil(T / lfr_n), ldx], ldx >= W */
  int32_t* out_lens;                                       /* [B] */
} mi355_sanm_input_args;
int mi355_sanm_input(const mi355_sanm_input_args* a, void* stream);

/* nn.log_softmax + mx.argmax over the vocabulary (sensevoice.py:437,451,468-493), one read of each row with an online maximum / sum of
 * exponentials.  Per row of logits [rows, ld >= V], any V >= 1:
 *   ids = the arg-max (the first maximum on ties, as mx.argmax);
 *   gap = max - the largest value at any OTHER index (0 on a tie, 0 for V = 1);
 *   lp  = the arg-max's log-probability, max - logsumexp = -log(sum_c exp(x_c - max));
 *   logp (nullable) [rows, ld_logp >= V] = (x_c - max) - log(sum_c exp(x_c - max)): a second pass over the row just read; logp may BE logits
 *   (in place, ld_logp == ld).
 * Finite logits are the caller's contract.  One workgroup per row: thread t sums the columns t, t + 256, ... in ascending order, the 256
 * partial sums are rescaled to the row maximum and joined by the wave butterfly and (w0 + w1) + (w2 + w3). */
typedef struct {
  const float* logits; int64_t ld; int64_t rows; int32_t V;
  int32_t* ids; float* gap; float* lp;                     /* [rows] each */
  float* logp; int64_t ld_logp;                            /* nullable */
} mi355_ctc_rows_args;
int mi355_ctc_rows(const mi355_ctc_rows_args* a, void* stream);

/* The collapse of _greedy_ctc_decode (sensevoice.py:450-463) on the rows skip .. lens[b] - 1 of ids [B, T] (row stride ld_ids >= T): drop
 * every row whose id equals the id of the row before it, then drop the blanks -- so a, blank, a keeps both a.  Row `skip` has no row before
 * it (the reference decodes log_probs[4:] on its own: an id equal to row skip - 1's still counts).  tokens [B, T] receives the kept ids in
 * order, counts [B] their number, frames [B, T] (nullable) the row index of each kept id (the first row of its run); the slots at and
 * beyond counts[b] hold -1.  lens NULL => T; lens[b] <= skip gives counts[b] = 0. */
typedef struct {
  const int32_t* ids; int64_t ld_ids;
  const int32_t* lens; int32_t skip; int32_t blank;
  int32_t B; int32_t T;
  int32_t* tokens; int32_t* counts; int32_t* frames;       /* [B, T] contiguous; [B]; [B, T] nullable */
} mi355_ctc_collapse_args;
int mi355_ctc_collapse(const mi355_ctc_collapse_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * MossFormer2 SE 48K (sts/models/mossformer2_se): the token shift with ScaleNorm, the FLASH gated single-head attention (global linear term and
 * grouped ReLU^2 term) and the gated FSMN memory (mossformer.hip).  Four entry points added to ABI 37 (new structs and functions only).
 * Plain float32, channels-last [B, T, ld] views with explicit row (ld) and batch strides, in floats.  lens [B] (device, nullable => T) is clamped
 * to [0, T]: rows t >= lens[b] READ as zero and are WRITTEN as zero.  No atomics, nothing allocated; every sum runs in an order that depends on
 * neither the launch geometry, nor B, nor the other items' lengths: two calls on the same bytes give the same bits, and an item inside a ragged
 * batch is bit-equal to that item alone.  Rows are 16-byte aligned (pointers multiples of 16 bytes, strides multiples of 4 floats).
 * Where a contract says that two tensors must not alias, the entry point compares their base pointers only: views that overlap without sharing
 * a base pointer are not detected and are the caller's duty.
 * ------------------------------------------------------------------------------------------ */
#define MI355_GAU_DIM 128         /* query / key width of the FLASH layer (to_qk's output) */
#define MI355_GAU_GROUP 256       /* rows per attention group */
#define MI355_GAU_ROPE_DIMS 32    /* leading columns that rotate, as the pairs (i, i + 16) */
#define MI355_GAU_MAX_E 2048      /* widest v | u */
#define MI355_GATED_FSMN_MAX_TAPS 63

/* The token shift of FLASH_ShareA_FFConvM.__call__ (flash_sharea_ffconvm.py:134-156) and ScaleNorm (scalenorm.py:35-41) in one read and one
 * write.  With s[b, t, c] = x[b, t - 1, c] for c < C / 2 (zero at t = 0) and x[b, t, c] for c >= C / 2 when shift != 0, s = x when shift == 0:
 *   y[b, t, c] = s * (g / max(sqrt(sum_c s^2) * C^-1/2, eps)),   g = *g (device scalar) or 1 when g is NULL.
 * An all-zero row gives exactly zero.  One wave per row: lane l adds the squares of its float4 pieces l, l + 64, ... in ascending order with
 * fmaf, then the xor butterfly.  C % 8 == 0, 8 <= C <= 2048, else MI355_ERR_ARG without a launch.  y must not alias x when shift != 0. */
typedef struct {
  const float* x; int64_t x_bstride; int64_t ldx;
  const float* g; float eps; int32_t shift;
  const int32_t* lens;
  int32_t B; int32_t T; int32_t C;
  float* y; int64_t y_bstride; int64_t ldy;
} mi355_shift_scalenorm_args;
int mi355_shift_scalenorm(const mi355_shift_scalenorm_args* a, void* stream);

/* The four heads of the FLASH layer are formed from qk [B, T, ldqk >= 128] (to_qk's output) wherever they are used (offsetscale.py:40-57,
 * mossformerblock_gfsmn.py:61-63: nn.RoPE(dims = 32, traditional = False, base = 10000)):
 *   head_h[t, i] = rope_t(qk[t, :] * gamma[h, :] + beta[h, :])[i],   h = 0 quad_q, 1 lin_q, 2 quad_k, 3 lin_k;   gamma, beta [4, 128]
 *   rope_t(z)[i] = z[i] cos[t, i] - z[i + 16] sin[t, i],  rope_t(z)[i + 16] = z[i + 16] cos[t, i] + z[i] sin[t, i]  for i < 16;  z[i] for i >= 32
 * with the host tables cos / sin [rope_rows >= T, 16] (device), cos[t, i] = cos(t * 10000^(-i / 16)); t is the row index inside the item.  The
 * four products of a pair are rounded on their own (no contraction).
 *
 * mi355_gau_kv: the global linear-attention matrix of cal_attention (flash_sharea_ffconvm.py:320-363),
 *   kv[b, d, e] = (sum_{t < lens[b]} lin_k[b, t, d] * vu[b, t, e]) / lens[b],   vu [B, T, ldvu >= E] (to_hidden's output, v | u), kv [B, 128, E].
 * Each group of 256 rows leaves its partial sum (an fmaf chain over its rows in ascending order, on v_mfma_f32_32x32x2_f32) in
 * ws [B, ceil(T / 256), 128, E] floats, caller-supplied; a second launch adds the partials of the groups below ceil(lens[b] / 256) in ascending
 * group order and divides by lens[b].  lens[b] == 0 gives kv = 0.  E % 64 == 0, 64 <= E <= 2048, T <= rope_rows, else MI355_ERR_ARG. */
typedef struct {
  const float* qk; int64_t qk_bstride; int64_t ldqk;
  const float* vu; int64_t vu_bstride; int64_t ldvu;
  const float* gamma; const float* beta;
  const float* rope_cos; const float* rope_sin; int32_t rope_rows;
  const int32_t* lens;
  int32_t B; int32_t T; int32_t E;
  float* ws; int64_t ws_floats;                /* >= B * ceil(T / 256) * 128 * E */
  float* kv; int64_t kv_bstride;               /* [B, 128, E], rows of E contiguous */
} mi355_gau_kv_args;
int mi355_gau_kv(const mi355_gau_kv_args* a, void* stream);

/* cal_attention and the output gate (flash_sharea_ffconvm.py:170-188,244-301,365-378; flash_attention_kernels.py:107-132), non-causal.  For
 * row t < lens[b] of group G = t / 256, over the keys j of the same group with j < lens[b], H = E / 2:
 *   S[t, j]   = relu(sum_d quad_q[t, d] * quad_k[j, d] / 256)^2
 *   A[t, e]   = sum_d lin_q[t, d] * kv[b, d, e] + sum_j S[t, j] * vu[j, e]      (the linear chain first, then the keys: the tile's fixed order)
 *   out[t, c] = (A[t, H + c] * vu[t, c]) * sigmoid(A[t, c] * vu[t, H + c]),   c < H;   out [B, T, ldo >= H]
 * The query tile of attn_tile.h: S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_32x32x2_f32, P fed from the accumulator registers; the score
 * tile never leaves the registers.  One workgroup owns 128 rows and cols columns of v with the same columns of u; cols = 0 lets the library
 * choose, 32 / 64 / 128 (a divisor of H) pins it: the bits do not depend on it.  qk_dim must be 128, group 256 and causal 0, else
 * MI355_ERR_UNSUPPORTED without a launch.  E % 64 == 0, 64 <= E <= 2048.  out must not alias vu. */
typedef struct {
  const float* qk; int64_t qk_bstride; int64_t ldqk;
  const float* vu; int64_t vu_bstride; int64_t ldvu;
  const float* kv; int64_t kv_bstride;
  const float* gamma; const float* beta;
  const float* rope_cos; const float* rope_sin; int32_t rope_rows;
  const int32_t* lens;
  int32_t B; int32_t T; int32_t E;
  int32_t qk_dim; int32_t group; int32_t causal; int32_t cols;
  float* out; int64_t out_bstride; int64_t ldo;
} mi355_gau_attention_args;
int mi355_gau_attention(const mi355_gau_attention_args* a, void* stream);

/* Gated_FSMN.__call__ behind its projections (gated_fsmn.py:105-116) with UniDeepFsmn's memory (unideepfsmn.py:96-123):
 *   y[b, t, c] = xv[b, t, c] * ((xu[b, t, c] + p[b, t, c]) + sum_{j < K} w[c, j] * p[b, t + j - (K - 1) / 2, c]) + res[b, t, c]
 * p = fsmn.project's output, xu = to_u's, xv = to_v's, res = the block's input; rows of p outside [0, lens[b]) read as zero.  The tap sum is
 * an fmaf chain from zero, j ascending; the last multiply-add is one fmaf.  w [C, K] float32 as mi355_dwconv takes it, K odd,
 * K <= MI355_GATED_FSMN_MAX_TAPS, else MI355_ERR_ARG without a launch.  y may alias res (each element is read, then written, by one thread);
 * y must not alias p. */
typedef struct {
  const float* p; int64_t p_bstride; int64_t ldp;
  const float* xu; int64_t xu_bstride; int64_t ldxu;
  const float* xv; int64_t xv_bstride; int64_t ldxv;
  const float* res; int64_t res_bstride; int64_t ldres;
  const float* w; int32_t K;
  const int32_t* lens;
  int32_t B; int32_t T; int32_t C;
  float* y; int64_t y_bstride; int64_t ldy;
} mi355_gated_fsmn_args;
int mi355_gated_fsmn(const mi355_gated_fsmn_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * FireRedASR2-AED (stt/models/fireredasr2/fireredasr2.py): the Conv2dSubsampling convs, the middle of the Conformer convolution module with its
 * LayerNorm over 2 x d_model channels, one step of the decoder's beam search and the decoder self-attention over a cache that is never
 * re-gathered (firered.hip).  Four entry points added to ABI 37 (new structs and functions only; no existing layout changed).  Plain float32,
 * no atomics, nothing allocated; every sum runs in a fixed order that depends on neither the launch geometry, nor the batch size, nor the other
 * items' lengths: two calls on the same bytes give the same bits, and an item inside a ragged batch is bit-equal to that item alone.  A call
 * that is refused (MI355_ERR_ARG / MI355_ERR_UNSUPPORTED) launches nothing and leaves every output untouched.
 * ------------------------------------------------------------------------------------------ */
#define MI355_SUBSAMPLE2D_MAX_COUT 64
/* The dense 3 x 3 / stride 2 convs of Conv2dSubsampling (fireredasr2.py:17-39): no padding, To = (T - 3) / 2 + 1, Fo = (F - 3) / 2 + 1,
 *   y[b, t, f, co] = act( bias[co] + sum_{kh, kw, ci} w[co, kh, kw, ci] * x[b, 2 t + kh, 2 f + kw, ci] ),
 * an fmaf chain from the bias in (kh, kw, ci) order.  x is [B, T, F] for Cin == 1 and channels-last [B, T, F, Cin] otherwise; w is
 * [Cout, 3, 3, Cin] (the reference's NHWC weight).  Input rows at or beyond lens_in[b] read as zero (the encoder's six zero frames of right
 * context arise this way for every item of a padded batch); output rows at or beyond lens_out[b] are written as zeros.  out_cf == 0 writes
 * y [B, To, Fo, Cout]; out_cf == 1 writes y [B, To, Cout, Fo], whose rows of Cout * Fo are in the reference's c * Fo + f order (what
 * Conv2dSubsampling.out reads after its transpose).  Cin is 1 or Cout; Cout a multiple of 4, <= MI355_SUBSAMPLE2D_MAX_COUT; T, F >= 3, else
 * MI355_ERR_ARG.  The weights are staged in LDS, Cout * 9 * Cin floats. */
typedef struct {
  const float* x; int64_t x_bstride;                     /* [B, T, F (, Cin)] */
  const float* w; const float* bias;                     /* [Cout, 3, 3, Cin]; [Cout] nullable => 0 */
  int32_t B; int32_t T; int32_t F; int32_t Cin; int32_t Cout; int32_t relu; int32_t out_cf;
  const int32_t* lens_in; const int32_t* lens_out;       /* [B] nullable => T / To */
  float* y; int64_t y_bstride;                           /* [B, To, Fo, Cout] or [B, To, Cout, Fo] */
} mi355_subsample2d_k3s2_args;
int mi355_subsample2d_k3s2(const mi355_subsample2d_k3s2_args* a, void* stream);

#define MI355_GLU_DWCONV_LN_MAX_TAPS 33
#define MI355_GLU_DWCONV_LN_MAX_C 2560
#define MI355_GLU_DWCONV_LN_ROWS 32     /* rows of one workgroup's tile (the register-window run of dw_window.h); half of it in launches of fewer than 256 such tiles */
/* ConformerConvolution.__call__ between its two pointwise convs (fireredasr2.py:111-116), channels-last.  x [B, L, 2 C] is pointwise conv 1's
 * output; with g[t, c] = x[t, c] * sigmoid(x[t, C + c]) for 0 <= t < lens[b] and 0 elsewhere:
 *   z[t, c] = sum_{k<K} w[c, k] * g[t + k - (K - 1) / 2, c]                       (no bias; an fmaf chain from zero, k ascending)
 *   n[t, c] = (z[t, c] - mean_t) / sqrt(var_t + eps) * ln_w[c] + ln_b[c]           (mean, then the mean of the squared deviations, over the C channels)
 *   y[t, c] = n * sigmoid(n)                                                       (full-precision expf)
 * rows lens[b] <= t < L are written as zeros.  One workgroup owns MI355_GLU_DWCONV_LN_ROWS rows across ALL C channels: z stays in registers
 * (thread i of NT holds the channels i, i + NT, ...; NT = 256 for C <= 1024 and 512 above, a function of C alone), so per row the traffic is
 * 2 C floats in (twice for K > 1: the halo of the neighbouring tile, from L2) and C floats out.  Each row statistic is summed per thread over
 * its channels in ascending order, per wave by the DPP sum, and over the waves as (w0 + w1) + (w2 + w3) (NT = 256) or serially from wave 0
 * (NT = 512).  The register window holds 1, 15 or 33 taps and a shorter kernel is centred in the next larger one with zero taps around it:
 * for K other than 1, 15 and 33 the rows up to 7 (K < 15) or 16 (K < 33) steps outside the kernel's own reach are read and gated too, and a
 * non-finite x there gives NaN (0 * inf) where the sum over K taps alone would not; finite x is the caller's contract.  K odd,
 * <= MI355_GLU_DWCONV_LN_MAX_TAPS; C a multiple of 4, <= MI355_GLU_DWCONV_LN_MAX_C; y must not alias x; else MI355_ERR_ARG. */
typedef struct {
  const float* x; int64_t x_bstride; int32_t ldx;        /* [B, L, ldx], ldx >= 2 C */
  const float* w;                                        /* [C, K] */
  const float* ln_w; const float* ln_b; float eps;       /* [C]; [C] */
  int32_t K; int32_t C; int32_t L; const int32_t* lens; int32_t B;   /* lens [B] nullable => L */
  float* y; int64_t y_bstride; int32_t ldy;              /* [B, L, ldy] */
} mi355_glu_dwconv_ln_swish_args;
int mi355_glu_dwconv_ln_swish(const mi355_glu_dwconv_ln_swish_args* a, void* stream);

#define MI355_BEAM_MAX 8
#define MI355_BEAM_MAX_V 65536
/* One step of TransformerDecoder.beam_search (fireredasr2.py:404-446) for N utterances of B beams, one workgroup per utterance.
 * `step[n]` is the length of the utterance's token history so far (the reference's ys.shape[1]: 1 after <sos>), so the histories hold <sos>
 * at index 0 and the host starts with step = 1, ind[n, j, 0] = j.  For every utterance whose done[n] == 0, in this order:
 *   u = logits[n * B + i, :] / smoothing;  t_c = log(exp(u_c - max u) / sum_c exp(u_c - max u) + 1e-10);  t_eos *= eos_penalty
 *   per beam i its B best (t, token), best first; a beam with finished[n, i] != 0 offers (0, eos), (-1e10, eos), ... instead
 *   the B best of the B x B sums scores[n, i] + t, best first: new beam j continues beam beam_idx[n, j] with token tok and value t
 *   scores[n, j] = the sum;  finished[n, j] = (tok == eos);  tokens_out[n, j, :step] = tokens_in[n, beam_idx, :step], tokens_out[n, j, step] = tok
 *   conf_out likewise with exp(t) at index step (nullable pair);  ind_out[n, j, :step] = ind_in[n, beam_idx, :step], ind_out[n, j, step] = j
 *   done[n] = 1 when all B beams are finished or step + 1 == max_steps[n];  step[n] += 1
 * An utterance with done[n] != 0 is left UNTOUCHED (no output of it is written, step[n] stays): the host may poll `done` every few steps, and the
 * final histories of utterance n are in the buffer that its last live step wrote.  An utterance whose step is outside [1, Tmax) only gets
 * done[n] = 1.  Selection: t is monotone in the logit, so the per-beam candidates are the B largest logits of the row with the eos column taken
 * out (V / 256 columns per thread, ascending; block_argmax), t is evaluated for those and for eos only, and eos is inserted by its (penalised) t.
 * TIES (the reference's argpartition leaves them unspecified): everywhere the larger value wins; among equal values the lower beam wins first, then
 * the lower token id (per beam: equal logits, or an equal t against eos, go to the lower token id; a finished beam's equal entries keep their order).
 * The max is exact; the sum of exponentials is per thread over its columns ascending, then the wave butterfly and (w0 + w1) + (w2 + w3).
 * 1 <= B <= MI355_BEAM_MAX, B < V <= MI355_BEAM_MAX_V, 0 <= eos_id < V, smoothing > 0, Tmax >= 2, the *_in and *_out buffers distinct, else
 * MI355_ERR_ARG. */
typedef struct {
  const float* logits; int64_t ld;                       /* [N * B, ld >= V] */
  int32_t N; int32_t B; int32_t V; int32_t Tmax;
  int32_t eos_id; float softmax_smoothing; float eos_penalty;
  float* scores; int32_t* finished;                      /* [N, B] each, in place */
  int32_t* step; const int32_t* max_steps; int32_t* done; /* [N] each; step and done in place */
  const int32_t* tokens_in; int32_t* tokens_out;         /* [N, B, Tmax] */
  const int32_t* ind_in; int32_t* ind_out;               /* [N, B, Tmax] */
  const float* conf_in; float* conf_out;                 /* [N, B, Tmax] nullable (together) */
  int32_t* beam_idx; int32_t* new_tokens; float* new_conf; /* [N, B] each; new_conf nullable */
} mi355_beam_step_args;
int mi355_beam_step(const mi355_beam_step_args* a, void* stream);

#define MI355_BEAM_ATTN_MAX_TK 4096
/* DecoderMultiHeadAttention.__call__ behind its projections (fireredasr2.py:272-279) for ONE query per (utterance, beam) over a k / v cache
 * that is never moved: the k / v rows of position s stay in the slot of the beam that produced them, and beam j of utterance n attends, for
 * 0 <= s <= pos[n], to row s of slot ind[n, j, s] (the table mi355_beam_step maintains; entries are clamped to [0, B)):
 *   p_s = softmax_s(scale * q . k[n, ind[n, j, s], s]),   out = sum_s p_s * v[n, ind[n, j, s], s]        (scale, softmax, then @ v)
 * per head h at columns [h dh, (h + 1) dh).  q / out are [N * B, ld] rows; the caches are [N * B slots, Tk rows, ld].  pos[n] is clamped to
 * Tk - 1; pos[n] < 0 (an utterance that is done) writes zero rows.  One wave per (utterance, beam, head): the scores of the keys s, s + 64, ...
 * per lane (an fmaf chain over dh), the exact max, the sum of exponentials per lane ascending and the wave butterfly, then an fmaf chain over
 * s ascending per output channel.  dh 64 or 128, any number of heads, 1 <= B <= MI355_BEAM_MAX, 1 <= Tk <= MI355_BEAM_ATTN_MAX_TK, Tk <= ld_ind,
 * rows 16-byte aligned (strides multiples of 4), else MI355_ERR_ARG. */
typedef struct {
  const float* q; int32_t ldq;                           /* [N * B, ldq] */
  const float* k; int64_t k_sstride; int32_t ldk;        /* slot n * B + i at k + (n * B + i) * k_sstride, rows [Tk, ldk] */
  const float* v; int64_t v_sstride; int32_t ldv;
  const int32_t* ind; int32_t ld_ind;                    /* [N, B, ld_ind] */
  const int32_t* pos;                                    /* [N] */
  int32_t N; int32_t B; int32_t Tk; int32_t heads; int32_t dh; float scale;
  float* out; int32_t ldo;                               /* [N * B, ldo] */
} mi355_beam_attention_args;
int mi355_beam_attention(const mi355_beam_attention_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Granite Speech NAR (stt/models/granite_speech_nar): block-local attention with Shaw relative positions, the self-conditioning softmax rows,
 * the posterior-weighted pooling and the projector's window assembly (granite_nar.hip).  Four entry points added to ABI 37 (new structs and
 * functions only; no existing layout changed).  Plain float32, no atomics, nothing allocated; every sum runs in a fixed order that depends on
 * neither the launch geometry, nor the batch size, nor the other items' lengths: two calls on the same bytes give the same bits, and an item
 * inside a ragged batch is bit-equal to that item alone.  lens [B] (device, nullable => T) is clamped to [0, T]; memory at and beyond lens[b]
 * is never read.  A call that is refused (MI355_ERR_ARG / MI355_ERR_UNSUPPORTED) launches nothing and leaves every output untouched.
 * ------------------------------------------------------------------------------------------ */
/* ConformerAttention.__call__ behind its projections (encoder.py:97-126).  Head h sits at columns [h dh, (h + 1) dh) of every row; the
 * tensors are NOT padded to a multiple of ctx.  With n = lens[b], for a query i < n of block m = i / ctx:
 *   s_ij = scale * ( q_i . k_j + q_i . table[max_pos + (i - j)] ),   out_i = sum_{m ctx <= j < (m + 1) ctx} softmax_j(s_i.) v_j,
 * where every key n <= j < (m + 1) ctx of that range is a ZERO key with a zero value that is NOT masked: its logit is the position term alone
 * and it takes softmax mass (the reference zero-pads the last block and to_kv has no bias).  Output rows n <= i < T are written as zeros.
 * table is [rows = 2 max_pos + 1, ldt >= dh], one table for all heads, row max_pos + d holding distance d = i - j, read in its own row order.
 * dh 64 or 128 (else MI355_ERR_UNSUPPORTED); ctx >= 1, max_pos >= ctx - 1 and rows == 2 max_pos + 1, else MI355_ERR_ARG.  Rows 16-byte
 * aligned (strides multiples of 4).  No [ctx, ctx] matrix is written to memory and there is no workspace. */
typedef struct {
  const float* q; int64_t q_bstride; int32_t ldq;        /* [B, T, ldq] */
  const float* k; int64_t k_bstride; int32_t ldk;
  const float* v; int64_t v_bstride; int32_t ldv;
  const float* table; int32_t ldt; int32_t rows; int32_t max_pos;   /* [rows, ldt] */
  const int32_t* lens; int32_t B; int32_t T; int32_t heads; int32_t dh; int32_t ctx; float scale;
  float* out; int64_t out_bstride; int32_t ldo;          /* [B, T, ldo] */
} mi355_shaw_block_attention_args;
int mi355_shaw_block_attention(const mi355_shaw_block_attention_args* a, void* stream);

#define MI355_SELFCOND_WAVE_MAX_V 256   /* up to here one wave owns a row (four rows per workgroup); above, one workgroup */
/* The self-conditioning step of ConformerEncoder.__call__ (encoder.py:280-281) per row of logits [rows, ld >= V], any V >= 1:
 *   probs[r, c] = expf(x_c - max) / sum_c expf(x_c - max),   p_blank[r] = probs[r, 0].
 * The maximum is exact; the sum is per thread over its columns t, t + NT, ... ascending (NT = 64 or 256 by V alone), then the wave butterfly
 * and, for NT = 256, (w0 + w1) + (w2 + w3).  Finite logits are the caller's contract. */
typedef struct {
  const float* logits; int64_t ld; int64_t rows; int32_t V;
  float* probs; int64_t ld_probs;                        /* [rows, ld_probs >= V] */
  float* p_blank;                                        /* [rows] */
} mi355_selfcond_rows_args;
int mi355_selfcond_rows(const mi355_selfcond_rows_args* a, void* stream);

/* _posterior_weighted_pool (encoder.py:302-334): out [B, ceil(T / window), ldo >= C].  With w_t = 1 - p_blank[b, t] for t < lens[b] and 0
 * beyond, per window n of frames n window .. min((n + 1) window, T) - 1:
 *   out[b, n, c] = sum_t h[b, t, c] * ( w_t / max(sum_t w_t, 1e-6) ),
 * the weights' sum in ascending order, the pooled value an fmaf chain from zero over t ascending.  A partial last window weights only its
 * real frames; a window wholly at or beyond lens[b] comes back zero. */
typedef struct {
  const float* h; int64_t h_bstride; int32_t ldh;        /* [B, T, ldh] */
  const float* p_blank; int64_t pb_bstride;              /* [B, T] */
  int32_t window; const int32_t* lens; int32_t B; int32_t T; int32_t C;
  float* out; int64_t out_bstride; int32_t ldo;          /* [B, ceil(T / window), ldo] */
} mi355_posterior_pool_args;
int mi355_posterior_pool(const mi355_posterior_pool_args* a, void* stream);

/* The window assembly of the projector (projector.py:190-215) in one launch, nblocks = ceil(T / block), nq = block / rate.  Row r of window
 * n of item b is h[b, n block + r] where that frame is below lens[b] and ZERO otherwise (the reference's right padding, before any add):
 *   kv[b nblocks + n, r, c]      = row_r[c] + positions[r, c]
 *   queries[b nblocks + n, g, c] = query[g, c] + ( sum_{i < rate} row_{g rate + i}[c] ) / rate        (the sum in ascending order)
 * query [nq, C], positions [block, C], queries [B nblocks, nq, C] and kv [B nblocks, block, C] are contiguous.  block a positive multiple of
 * rate, else MI355_ERR_ARG. */
typedef struct {
  const float* h; int64_t h_bstride; int32_t ldh;        /* [B, T, ldh] */
  const int32_t* lens; int32_t B; int32_t T; int32_t C; int32_t block; int32_t rate;
  const float* query; const float* positions;            /* [block / rate, C]; [block, C] */
  float* queries; float* kv;                             /* [B nblocks, block / rate, C]; [B nblocks, block, C] */
} mi355_qformer_windows_args;
int mi355_qformer_windows(const mi355_qformer_windows_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355AUDIO_H */
